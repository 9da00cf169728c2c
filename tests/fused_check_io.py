"""The Python half of gaussian-lic_amd/shim/fused_check_io.h, the file protocol of the shim/fused_*_check programs: raw little-endian arrays
under one directory, written here with numpy's tofile and read back with numpy's fromfile.
  inputs   {xyz,scaling,rotation,opacity,dc,rest}.f32 (the six raw parameter groups of P rows; rest only at SH degree > 0),
           {view,proj,campos}<tag>.f32 (one camera; tags "", "2", ...), scalars.f32 (tanfovx, tanfovy, 4 lims of the first camera, then whatever
           the program documents) and, when present, gt.f32 and tie_rank.f32 (the rows' original indices of a map handed over in a permuted
           order, as floats); everything else is the program's own
  outputs  out_<name>: out_{xyz,dc,rest,opacity,scaling,rotation}.f32, out_m_<name>.f32, out_v_<name>.f32 and out_tie.i32 are the 19 row
           arrays (dump_rows); everything else is the program's own
No GPU and no compiled program is needed to import this module or to write and read the files."""
import functools
import importlib.util
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = (("xyz", "xyz"), ("scaling", "scaling"), ("rotation", "rotation"), ("opacity", "opacity"), ("features_dc", "dc"), ("features_rest", "rest"))
ROW_NAMES = ("xyz", "dc", "rest", "opacity", "scaling", "rotation")   # kNames of the header


@functools.lru_cache(maxsize=None)
def build_shim():
    """gaussian-lic_amd/shim/build_shim.py as a module (loaded once per process)."""
    spec = importlib.util.spec_from_file_location("build_shim", os.path.join(ROOT, "gaussian-lic_amd", "shim", "build_shim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(name):
    """The path of the program `name` of build_shim.FUSED_CHECKS, built when missing or stale (a build failure fails)."""
    exe = build_shim().build_fused_check(name)
    assert os.path.exists(exe)
    return exe


def _numpy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else t


def write(d, name, a, dtype=np.float32, ext="f32"):
    np.ascontiguousarray(_numpy(a), dtype).tofile(os.path.join(d, f"{name}.{ext}"))


def write_inputs(d, model_or_tensors, cams, scalars_extra=(), gt=None, tie_rank=None, **arrays):
    """The inputs check_io::read_inputs reads, from a GaussianModel or a dict of raw parameter tensors and one camera or a sequence of them
    (the first untagged, then "2", "3", ...); `arrays` are further float32 files <key>.f32."""
    src = model_or_tensors
    for k, n in GROUPS:
        t = src[k] if isinstance(src, dict) else getattr(src, k)
        if n != "rest" or t.numel():
            write(d, n, t)
    cams = list(cams) if isinstance(cams, (list, tuple)) else [cams]
    for i, cam in enumerate(cams):
        tag = "" if i == 0 else str(i + 1)
        write(d, "view" + tag, cam.world_view_transform); write(d, "proj" + tag, cam.full_proj_transform); write(d, "campos" + tag, cam.camera_center)
    cam = cams[0]
    write(d, "scalars", np.array([cam.tanfovx, cam.tanfovy, cam.limx_neg, cam.limx_pos, cam.limy_neg, cam.limy_pos, *scalars_extra], np.float32))
    if gt is not None:
        write(d, "gt", gt)
    if tie_rank is not None:
        write(d, "tie_rank", tie_rank)
    for name, a in arrays.items():
        write(d, name, a)


def run(exe, *args, timeout=300, env=None):
    """One fresh child process of the program; asserts that it exited with 0 and returns the completed process."""
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def read(d, name, dtype):
    return torch.from_numpy(np.fromfile(os.path.join(d, "out_" + name), dtype))


def read_rows(d, M, tie=False):
    """The row arrays check_io::dump_rows wrote, as flat int32 tensors (the bits) keyed as the header names them: "xyz", "m_xyz", "v_xyz", ...
    (rest only when M > 0) and, with tie=True, "tie"."""
    rows = {pre + n: read(d, pre + n + ".f32", np.int32) for n in ROW_NAMES if n != "rest" or M > 0 for pre in ("", "m_", "v_")}
    if tie:
        rows["tie"] = read(d, "tie.i32", np.int32)
    return rows
