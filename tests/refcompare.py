"""HIP path vs the REFERENCE's own kernels (oracle/_ref/libref_hip.so) on the same MI355X and the same inputs: one function that
runs both and returns every count the parity gate needs — integer-stage mismatches, the exact number of elements over the 1e-4
bar, the maximum error, and (scenes small enough for the CPU oracle) the worst stratum ratio of the row-wise comparison of tests/rowwise.py —
for the fast and the strict arithmetic of the blend kernels.  Shared by
tests/test_fullsize_reference_gpu.py (asserts) and tests/parity_report.py (prints / writes profiles/*parity*.json).
Test infrastructure: imports oracle/ (the checker)."""
import numpy as np

TOL = 1e-4
GRADS = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_ddc", "dL_dsh", "dL_dscale", "dL_drot")


def _err_stats(got, ref, scale=None, keep_over=False):
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    if ref.size == 0:
        return dict(n=0, over=0, max_rel=0.0, bit_equal=True)
    scale = max(float(np.abs(ref).max()), 1e-30) if scale is None else scale
    err = np.abs(got - ref) / scale
    out = dict(n=int(ref.size), over=int((err > TOL).sum()), max_rel=float(err.max()), bit_equal=bool(np.array_equal(got, ref)))
    if keep_over and out["over"]:
        out["_over_idx"], out["_scale"] = np.nonzero(err > TOL)[0], scale
        out["_got_over"] = got[out["_over_idx"]]
    return out


PROBE_MAX_P = 80000      # the conditioning probe runs the CPU oracle twice: small scenes only
ILL_CONDITIONED = 1e-5   # fp32 (sequential C oracle) vs fp64 at the element, relative to the tensor's max-abs
REF_RUNS = 8             # further runs of the reference's OWN kernels an over-element is held against (its backward sums with atomics: every run is a
                         # slightly different answer — up to 5e-5 of a tensor's max-abs apart; the HIP backward is deterministic)


def conditioning_probe(st, sc, camd, dL, scale_modifier, lambda_erank=0.0, ref_runs=None):
    """For every gradient of `st` with elements beyond 1e-4: how many of THOSE elements are ill-conditioned in fp32, i.e. the fp32 C oracle — the
    reference's arithmetic in sequential order — is itself more than 1e-5 of the tensor's max-abs away from the double-precision oracle on the same
    inputs.  Adds st[k]["over_ill_conditioned"] and st[k]["fp32_vs_fp64_at_over"]; drops the private index arrays.
    ref_runs = [run 1, run 2, ...] of the reference's own kernels on the same inputs.  The reference's backward accumulates with atomicAdd: the order of
    its sums, hence their last bits, changes from run to run (the same scene, the same element: 6.4e-5 ... 1.03e-4 away from the deterministic HIP value
    in twelve runs, profiles/r06ag_pose_case20_*.log), so "within 1e-4 of the reference" is held against the reference's outputs, plural: an element
    over the bar against run 1 does not count when it is within the bar of another run.  st[k]["over_within_other_run"], st[k]["err_per_run_at_over"]
    (first element), st[k]["over_hip_closer_to_fp64"] = the over-elements at which the HIP value is at least as close to the double-precision oracle as the
    reference's run is, and st[k]["over_excused"] = the over-elements that are ill-conditioned OR within 1e-4 of another run of the reference OR closer
    to fp64 than the reference.  Reported by summarize(), never absorbed."""
    from oracle.oracle import Oracle, build
    need = [k for k in GRADS if k in st and "_over_idx" in st[k]]
    if need:
        build()
        sc = dict(sc, scale_modifier=scale_modifier)
        g = {}
        for dt in (np.float32, np.float64):
            o = Oracle(dt)
            f = o.forward(sc, camd)
            g[dt] = o.backward(sc, camd, f, dL, lambda_erank=lambda_erank)
        for k in need:
            idx, scale = st[k]["_over_idx"], st[k]["_scale"]
            a, b = np.asarray(g[np.float32][k], np.float64).reshape(-1)[idx], np.asarray(g[np.float64][k], np.float64).reshape(-1)[idx]
            e = np.abs(a - b) / scale
            ill = e > ILL_CONDITIONED
            st[k]["over_ill_conditioned"] = int(ill.sum())
            st[k]["fp32_vs_fp64_at_over"] = [float(f"{v:.2e}") for v in e[:8]]
            # where the HIP value is at least as close to the double-precision oracle as the reference's run is, the gap to the reference is mostly the
            # reference's own error (case 20 of the posed suite: HIP 3.3e-5 from fp64, the reference's run 7.1e-5, on opposite sides)
            e_hip = np.abs(st[k]["_got_over"] - b) / scale
            st[k]["hip_vs_fp64_at_over"] = [float(f"{v:.2e}") for v in e_hip[:8]]
            closer = np.zeros_like(ill)
            if ref_runs is not None:
                e_ref = np.abs(np.asarray(ref_runs[0][k], np.float64).reshape(-1)[idx] - b) / scale
                st[k]["ref_vs_fp64_at_over"] = [float(f"{v:.2e}") for v in e_ref[:8]]
                closer = e_hip <= e_ref
                st[k]["over_hip_closer_to_fp64"] = int(closer.sum())
            unstable = np.zeros_like(ill)
            if ref_runs is not None and len(ref_runs) > 1:
                got = st[k]["_got_over"]
                errs = np.stack([np.abs(got - np.asarray(r[k], np.float64).reshape(-1)[idx]) / scale for r in ref_runs])   # [runs, over-elements]
                unstable = errs[1:].min(axis=0) <= TOL
                st[k]["over_within_other_run"] = int(unstable.sum())
                st[k]["err_per_run_at_over"] = [float(f"{v:.2e}") for v in errs[:, 0]]
            st[k]["over_excused"] = int((ill | unstable | closer).sum())
    for k in GRADS:
        if k in st:
            st[k].pop("_over_idx", None); st[k].pop("_scale", None); st[k].pop("_got_over", None)


def _fp64_rows(sc, camd, dL, scale_modifier):
    """(the double-precision oracle's gradients, its visibility mask) on the inputs of compare()."""
    from oracle.oracle import Oracle, build
    build()
    o = Oracle(np.float64)
    sc = dict(sc, scale_modifier=scale_modifier)
    f = o.forward(sc, camd)
    return o.backward(sc, camd, f, dL), f["pre"]["radii"] > 0


PATH_KERNELS = {"atomic": ("tile_hist", "tile_scan", "tile_bin"), "radix": ("sort_hist", "sort_scatter", "finalize_lists")}


def compare(kind, P, W, H, deg, seed, modes=("fast", "strict"), backward=True, view=None, sigma_scale=1.0, scale_modifier=1.0, binning="radix", morton=False):
    """Returns {"scene":…, "ref": {...unit counts}, "<mode>": {stage: stats}}.  P must be a multiple of 256 (with a partial last block
    the reference's duplicateWithKeys races pad keys over the last Gaussian's slots, rasterizer_impl.cu:73-131).
    view / sigma_scale: conftest.make_scene (camera pose: identity, a config-4 view, a general SE(3) pose; extent of the Gaussians);
    scale_modifier: the rasterizer setting of renderer.h:36 / forward.cu:120-149, passed to both sides.
    binning: "radix" | "atomic" — how the HIP forward groups the instances by tile, FORCED (gslic_set_binning_mode; never `auto`, whose choice
    depends on what the thread's earlier forwards measured) and then VERIFIED: st["binning_path"] is what gslic_get_binning_path reports and
    st["path_launches"] the launch counts of the two paths' kernels from the library's profiler — the caller asserts on them.
    morton: the HIP side gets the map's rows PERMUTED into Morton order (trainer.morton_order) with tie_rank = the rows' original indices — what
    trainer.GaussianModel(order="morton"), i.e. bench.py's timed configuration, hands the kernels; the reference gets the rows in the original
    order (rasterizer_impl.cu:395-424 defines the order of the lists on those).  Per-Gaussian outputs are un-permuted and the lists' Gaussian
    ids mapped back to original indices before anything is compared."""
    import torch
    from conftest import make_scene
    from gpu_helpers import hip_backward, hip_forward, npy
    from gaussian_lic_amd import _lib
    from gaussian_lic_amd.synthetic import pixel_grad
    from oracle.ref_build import refkernels
    assert P % 256 == 0 and binning in PATH_KERNELS
    rk = refkernels.RefKernels()
    from conftest import clamp_masked_visible
    raw, sc, camd, cam = make_scene(kind, P, W, H, deg, seed, view=view, sigma_scale=sigma_scale)
    dL = pixel_grad(H, W, seed=1)
    ref = rk.run(sc, camd, dL.numpy() if backward else None, scale_modifier=scale_modifier)
    vis = ref["radii"] > 0
    out = dict(scene=dict(kind=kind, P=P, W=W, H=H, deg=deg, seed=seed, view=view, sigma_scale=sigma_scale, scale_modifier=scale_modifier,
                          binning=binning, morton=bool(morton)),
               ref=dict(R=int(ref["R"]), B32=int(ref["B"]), visible=int(vis.sum()), clamp_masked_visible=clamp_masked_visible(sc, camd, ref["radii"])))
    perm = tie = None
    if morton:
        from gaussian_lic_amd import trainer
        perm = trainer.morton_order(raw["xyz"])                      # storage row s holds original row perm[s]
        tie = perm.to(torch.int32).to("cuda:0")
    # the HIP side's inputs: the SAME activated values the reference gets (activated once, in the original order: LibTorch's CPU reductions need not
    # give a row the same last bit at every position of a tensor), then the rows permuted
    from gaussian_lic_amd.synthetic import activate
    act = activate(raw)
    if morton:
        act = {k: (v[perm].contiguous() if torch.is_tensor(v) else v) for k, v in act.items()}
        perm = perm.numpy()

    def unperm(a):   # per-Gaussian array in storage order -> original order
        if perm is None:
            return a
        o = np.empty_like(a)
        o[perm] = a
        return o

    rows64 = None
    prev_binning = _lib.set_binning_mode(binning)
    try:
        for mode in modes:
            prev = _lib.set_math_mode(mode == "strict")
            try:
                _lib.profile_enable(True, only=[k for ks in PATH_KERNELS.values() for k in ks])
                _lib.profile_reset()
                got = hip_forward(raw, cam, export=("tiles_touched", "means2D", "depths", "conic_opacity", "rgb", "point_list", "ranges",
                                                    "n_contrib"), scale_modifier=scale_modifier, tie_rank=tie, act=act)
                launches = {k: v[1] for k, v in _lib.profile_collect().items()}
                _lib.profile_enable(False)
                d = got["dbg"]
                st = {}
                st["binning_path"] = _lib.binning_path()[0]
                st["path_launches"] = {p_: int(sum(launches.get(k, 0) for k in ks)) for p_, ks in PATH_KERNELS.items()}
                tt_h = unperm(npy(d["tiles_touched"]).astype(np.uint32))
                bad = np.nonzero(tt_h != ref["tiles_touched"])[0]
                st["radii_mismatch"] = int((unperm(npy(got["radii"])) != ref["radii"]).sum())
                st["tiles_touched_mismatch"] = int(bad.size)
                st["R"] = int(got["R"])
                pl_h, pl_r = npy(d["point_list"]).astype(np.uint32), ref["point_list"]
                if perm is not None:
                    pl_h = perm[pl_h].astype(np.uint32)
                if bad.size:
                    pl_h, pl_r = pl_h[~np.isin(pl_h, bad)], pl_r[~np.isin(pl_r, bad)]
                st["point_list_equal"] = bool(pl_h.shape == pl_r.shape and np.array_equal(pl_h, pl_r))
                st["ranges_equal"] = bool(np.array_equal(npy(d["ranges"]).astype(np.uint32), ref["ranges"])) if not bad.size else None
                for k, rkey in (("means2D", "means2D"), ("depths", "depths"), ("conic_opacity", "conic_opacity"), ("rgb", "rgb")):
                    st[k + "_bit_equal"] = bool(np.array_equal(unperm(npy(d[k]))[vis], ref[rkey][vis]))
                st["color"] = _err_stats(npy(got["color"]), ref["color"])
                st["final_T"] = _err_stats(npy(got["final_T"]), ref["final_T"])
                nc = npy(d["n_contrib"]).astype(np.uint32)
                st["n_contrib_mismatch"] = int((nc != ref["n_contrib"]).sum())
                st["pixels"] = int(nc.size)
                if backward:
                    g = hip_backward(got, dL)
                    for k in GRADS:
                        scale = None
                        if k == "dL_drot":   # unnormalised-quaternion gradient: scale of the chain it belongs to (as test_vs_reference_kernels_gpu.py)
                            scale = max(float(np.abs(ref["dL_drot"]).max()), float(np.abs(ref["dL_dscale"]).max() * sc["scales"].max()), 1e-30)   # (a view that sees nothing: all zeros)
                        st[k] = _err_stats(unperm(g[k]), ref[k], scale, keep_over=(mode == "strict" and P <= PROBE_MAX_P))
                    if P <= PROBE_MAX_P:
                        # reported next to the max-abs figures, never asserted: the worst stratum ratio of the row-wise comparison (tests/rowwise.py) —
                        # HIP error / the reference run's error per decade of row magnitude, both against the double-precision oracle
                        if rows64 is None:
                            rows64 = _fp64_rows(sc, camd, dL.numpy(), scale_modifier)
                        import rowwise
                        cmp = rowwise.compare({k: unperm(g[k]) for k in GRADS}, ref, rows64[0], vis & rows64[1], P, GRADS)
                        for k, best in rowwise.worst_per_tensor(cmp, ("median", "p90") if mode == "strict" else ("median",)).items():
                            st[k]["rowwise_worst"] = [float(f"{best[0]:.3g}"), int(best[1]), best[2]]
                    if mode == "strict" and P <= PROBE_MAX_P:
                        # (only when an element is over the bar: further runs of the reference's kernels, whose atomics make every run a slightly
                        # different answer — the element counts when it is over the bar against every one of them)
                        again = None
                        if any("_over_idx" in st[k] for k in GRADS):
                            again = [ref]
                            for _ in range(REF_RUNS):
                                again.append(rk.run(sc, camd, dL.numpy(), scale_modifier=scale_modifier))
                                if all(("_over_idx" not in st[k]) or
                                       (np.abs(st[k]["_got_over"] - np.asarray(again[-1][k], np.float64).reshape(-1)[st[k]["_over_idx"]]) / st[k]["_scale"] <= TOL).all()
                                       for k in GRADS):
                                    break
                        conditioning_probe(st, sc, camd, dL.numpy(), scale_modifier, ref_runs=again)
                out[mode] = st
                del got
                torch.cuda.empty_cache()
            finally:
                _lib.profile_enable(False)
                _lib.set_math_mode(prev)
    finally:
        _lib.set_binning_mode(prev_binning)
    return out


def assert_path(res):
    """The HIP forward of every mode of `res` took the grouping the comparison FORCED: the library says so (gslic_get_binning_path) and only that
    path's kernels were launched (profiler counts).  Above GS_TILE_BIN_MAX_T = 36 864 tiles the atomic path does not exist."""
    want = res["scene"]["binning"]
    other = "radix" if want == "atomic" else "atomic"
    for mode in ("fast", "strict"):
        if mode in res and res["ref"]["R"] > 0:
            st = res[mode]
            assert st["binning_path"] == want, (mode, st["binning_path"], want)
            assert st["path_launches"][want] > 0 and st["path_launches"][other] == 0, (mode, st["path_launches"])


def compare_reference_builds(kind, P, W, H, deg, seed):
    """The yardstick: the reference's kernels against THEMSELVES under the two contraction settings — oracle/_ref/libref_hip.so
    (-ffp-contract=off, the pin of the parity tests) vs libref_hip_fma.so (-ffp-contract=fast: hipcc's default and the analogue of nvcc's
    default --fmad=true that upstream is built with).  Same statistics as compare(): what one compiler flag moves in the reference's own
    output is the noise floor any "bit-identical to the reference" statement sits on."""
    from conftest import make_scene
    from gaussian_lic_amd.synthetic import pixel_grad
    from oracle.ref_build import refkernels
    assert P % 256 == 0
    raw, sc, camd, cam = make_scene(kind, P, W, H, deg, seed)
    dL = pixel_grad(H, W, seed=1).numpy()
    a = refkernels.RefKernels().run(sc, camd, dL)
    b = refkernels.RefKernels(fma=True).run(sc, camd, dL)
    vis = (a["radii"] > 0) & (b["radii"] > 0)
    st = {}
    st["radii_mismatch"] = int((a["radii"] != b["radii"]).sum())
    bad = np.nonzero(a["tiles_touched"] != b["tiles_touched"])[0]
    st["tiles_touched_mismatch"] = int(bad.size)
    st["R"] = [int(a["R"]), int(b["R"])]
    pa, pb = a["point_list"], b["point_list"]
    st["point_list_equal_raw"] = bool(pa.shape == pb.shape and np.array_equal(pa, pb))
    if bad.size:
        pa, pb = pa[~np.isin(pa, bad)], pb[~np.isin(pb, bad)]
    st["point_list_equal"] = bool(pa.shape == pb.shape and np.array_equal(pa, pb))   # after removing the Gaussians whose tile count differs
    st["point_list_order_differences"] = int((pa != pb).sum()) if pa.shape == pb.shape else None
    for k in ("means2D", "depths", "conic_opacity", "rgb"):
        st[k + "_bit_equal"] = bool(np.array_equal(a[k][vis], b[k][vis]))
        st[k + "_elements_differing"] = int((a[k][vis] != b[k][vis]).sum())
    st["color"] = _err_stats(b["color"], a["color"])
    st["final_T"] = _err_stats(b["final_T"], a["final_T"])
    st["n_contrib_mismatch"] = int((a["n_contrib"] != b["n_contrib"]).sum())
    st["pixels"] = int(a["n_contrib"].size)
    for k in GRADS:
        scale = None
        if k == "dL_drot":
            scale = max(float(np.abs(a["dL_drot"]).max()), float(np.abs(a["dL_dscale"]).max() * sc["scales"].max()))
        st[k] = _err_stats(b[k], a[k], scale)
    return st


def summarize_reference_builds(st):
    parts = [f"radii!={st['radii_mismatch']}", f"tiles_touched!={st['tiles_touched_mismatch']}", f"R={st['R']}",
             f"lists_equal={st['point_list_equal']} (order differences {st['point_list_order_differences']})",
             "geometry elements differing: " + ", ".join(f"{k}={st[k + '_elements_differing']}" for k in ("means2D", "depths", "conic_opacity", "rgb")),
             f"color over1e-4={st['color']['over']}/{st['color']['n']} max={st['color']['max_rel']:.2e} bit_equal={st['color']['bit_equal']}",
             f"final_T over={st['final_T']['over']} max={st['final_T']['max_rel']:.2e}", f"n_contrib!={st['n_contrib_mismatch']}/{st['pixels']}"]
    for k in GRADS:
        parts.append(f"{k} over={st[k]['over']}/{st[k]['n']} max={st[k]['max_rel']:.2e}")
    return "  [reference -ffp-contract=fast vs reference -ffp-contract=off] " + "  ".join(parts)


def summarize(res):
    """One line per mode: what a reader of the test log needs."""
    lines = []
    s = res["scene"]
    pose = "" if s.get("view") is None else f" view={s['view']}"
    pose += "" if s.get("sigma_scale", 1.0) == 1.0 else f" sigma_scale={s['sigma_scale']}"
    pose += "" if s.get("scale_modifier", 1.0) == 1.0 else f" scale_modifier={s['scale_modifier']}"
    pose += f" [binning forced: {s.get('binning')}; rows: {'Morton order + tie_rank' if s.get('morton') else 'insertion order'}]"
    lines.append(f"{s['kind']} P={s['P']} {s['W']}x{s['H']} deg{s['deg']} seed={s['seed']}{pose}: R={res['ref']['R']} visible={res['ref']['visible']} "
                 f"clamp-masked visible={res['ref'].get('clamp_masked_visible')}")
    for mode in ("fast", "strict"):
        if mode not in res:
            continue
        st = res[mode]
        npx = st["pixels"]
        parts = [f"path={st.get('binning_path')} launches={st.get('path_launches')}",
                 f"radii!={st['radii_mismatch']}", f"tiles_touched!={st['tiles_touched_mismatch']}", f"lists_equal={st['point_list_equal']}",
                 f"geom_bits={'ok' if all(st[k + '_bit_equal'] for k in ('means2D', 'depths', 'conic_opacity')) else 'DIFF'}",
                 f"rgb_bits={'ok' if st['rgb_bit_equal'] else 'diff'}",
                 f"color over1e-4={st['color']['over']}/{st['color']['n']} max={st['color']['max_rel']:.2e} bit_equal={st['color']['bit_equal']}",
                 f"final_T over={st['final_T']['over']} max={st['final_T']['max_rel']:.2e}",
                 f"n_contrib!={st['n_contrib_mismatch']}/{npx}"]
        for k in GRADS:
            if k in st:
                ill = f" (ill-conditioned in fp32: {st[k]['over_ill_conditioned']}, fp32 vs fp64 there {st[k]['fp32_vs_fp64_at_over']}, HIP vs fp64 {st[k].get('hip_vs_fp64_at_over')}, reference vs fp64 {st[k].get('ref_vs_fp64_at_over')}" + (f"; against {len(st[k]['err_per_run_at_over'])} runs of the reference's atomics the first of them is {st[k]['err_per_run_at_over']} away: {st[k]['over_within_other_run']} within 1e-4 of another run, {st[k].get('over_hip_closer_to_fp64', 0)} closer to fp64 than the reference" if "over_within_other_run" in st[k] else "") + ")" if "over_ill_conditioned" in st[k] else ""
                rw_ = st[k].get("rowwise_worst")
                rw_ = "" if rw_ is None else (f" rowwise x{rw_[0]:.2f}@1e-{rw_[1]}/{rw_[2]}" if rw_[1] >= 0 else " rowwise -")
                parts.append(f"{k} over={st[k]['over']}/{st[k]['n']} max={st[k]['max_rel']:.2e}{rw_}{ill}")
        lines.append(f"  [{mode}] " + "  ".join(parts))
    return "\n".join(lines)
