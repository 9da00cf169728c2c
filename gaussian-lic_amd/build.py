"""Builds libgslic_hip.so in-tree with hipcc for gfx950 (no torch, no hipify, no CMake).

    python gaussian-lic_amd/build.py [--force] [--verbose]

Every .hip file is compiled to an object in csrc/build/ (in parallel) and linked into
gaussian-lic_amd/libgslic_hip.so.  preprocess.hip is compiled with -ffp-contract=off: it holds the
integer-deciding canonical arithmetic that must match the oracle bit for bit.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
LIB = os.path.join(HERE, "libgslic_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

SOURCES = {
    "api.hip": [],
    "scan.hip": [],
    "radix_sort.hip": [],
    "tile_bin.hip": [],
    "preprocess.hip": ["-ffp-contract=off"],
    "render.hip": ["-fno-slp-vectorize"],
    "render_bwd_scan.hip": ["-fno-slp-vectorize"],
    "preprocess_bwd.hip": [],
    "preprocess_bwd_gstat.hip": [],   # the gradient-statistics variants of preprocess_bwd.hip's kernels, in a module of their own (their rule pins its own rounding: fp contract(off))
    "preprocess_bwd_cam_adam.hip": [],   # the camera gradient with the fused Adam (depth chain variant, its tail, the checked reduction), in a module of its own like the statistics variants
    "adam.hip": [],
    "ssim.hip": ["-ffp-contract=off"],   # the maps are held bit-exact to the reference kernels under the same flag (tests/golden/ssim_*.npz)
    "depth_loss.hip": [],    # its two kernels pin their own rounding (fp contract(off)): the gradient is held to autograd's bits
    "exposure.hip": ["-ffp-contract=off"],   # the 3x4 exposure model: every product and sum of the rule rounded on its own, apply and dL_dimage tested on bits
    "keyframes.hip": ["-ffp-contract=off"],  # the keyframe store: integer sums and one float multiply (decode), one product rounded on its own (encode), tested on bits
    "keyframes_depth.hip": ["-ffp-contract=off"],  # the store's depth slabs, in a module of their own: an integer minimum and one exact multiply (decode), one exact product, an add and a floor (encode)
    "pose.hip": ["-ffp-contract=off"],       # the pose set's step: every float32 product and sum of the rule rounded on its own, in the header's order
    "pose_shared.hip": ["-ffp-contract=off"],   # the shared extrinsic / time-offset step and the row calibration: the same rule, rounded the same way
    "covis.hip": [],         # covisibility bits: integer loads, stores, popcounts and atomic adds only: no arithmetic a flag could change
    "knn.hip": [],
    "extend.hip": ["-ffp-contract=off"],  # pixel assignment decides integers: canonical order like preprocess.hip
    "prune.hip": [],         # comparisons and copies only: no arithmetic a flag could change
    "row_ops.hip": [],       # the segmented row kernel of prune and densify: copies, zeros and comparisons only
    "morton.hip": ["-ffp-contract=off"],   # the key rule of gslic_morton_order: every float32 step rounded on its own, tested on bits
    "contrib.hip": ["-ffp-contract=off"],  # replays the strict blend: every product of the power and of w = alpha T is rounded on its own
    "densify.hip": ["-ffp-contract=off"],  # the split children's positions: every product and sum rounded on its own, as the header writes them
    "lidar_depth.hip": ["-ffp-contract=off"],  # pixel assignment decides integers, and the near bound is tested on bits: every step rounded on its own
}
COMMON = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-Wno-inline-asm",
          "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function"]
HEADERS = ["gslic_common.h", "kernels.h", "render_fwd_body.inc", "preprocess_bwd_body.inc", "preprocess_bwd_device.inc", "contrib_body.inc", "loss_bwd_body.inc", "row_rules.h", "keyframe_rows.h", os.path.join("..", "..", "include", "gslic_hip.h")]


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force=False, verbose=False):
    # A/B variants (tools/ab): GSLIC_BUILD_EXTRA="-DFOO=1 ..." compiles every file with extra flags into its own object directory and
    # GSLIC_BUILD_LIB=<path> names the library, so the in-tree libgslic_hip.so is left alone
    global OBJ, LIB
    extra_all = os.environ.get("GSLIC_BUILD_EXTRA", "").split()
    if os.environ.get("GSLIC_BUILD_LIB"):
        LIB = os.path.abspath(os.environ["GSLIC_BUILD_LIB"])
        OBJ = os.path.join(CSRC, "build_" + os.path.splitext(os.path.basename(LIB))[0])
        force = True
    os.makedirs(OBJ, exist_ok=True)
    hdr_paths = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    jobs = []
    for src, extra in SOURCES.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        if force or _newer(s, o) or any(_newer(h, o) for h in hdr_paths):
            jobs.append((s, o, [HIPCC] + COMMON + extra + extra_all + ["-c", s, "-o", o]))

    def run(job):
        s, o, cmd = job
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        return s, r

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        for s, r in ex.map(run, jobs):
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise RuntimeError(f"hipcc failed on {s}")
            if verbose and r.stderr.strip():
                sys.stderr.write(r.stderr)
    objs = [os.path.join(OBJ, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or not os.path.exists(LIB):
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise RuntimeError("link of libgslic_hip.so failed")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
