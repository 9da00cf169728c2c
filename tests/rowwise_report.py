"""Prints (run on the MI355X: `python tests/rowwise_report.py [out.txt]`) the stratified row-wise comparison of every case and path of
tests/test_rowwise_gradients_gpu.py: tensor x stratum x (n, fp32-oracle median / p90, HIP median / p90, ratios), all against the fp64 oracle,
then the largest judged ratio per path.  rowwise.FACTOR is derived from its last lines; profiles/rowwise_gradient_strata.txt is its output.
Asserts nothing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out_path=None):
    import rowwise as rw
    from oracle.oracle import Oracle, build
    from test_rowwise_gradients_gpu import PATHS, references, run_path
    build()
    o32, o64 = Oracle(np.float32), Oracle(np.float64)
    lines, top = [], {}
    for name in rw.CASES:
        c = references(name, o32, o64)
        lines.append(f"## {name}: {int(c['vis'].sum())} visible of {c['P']} Gaussians; share of the non-zero rows wholly below 1e-4 / 1e-2 of the tensor's "
                     "max-abs: " + "  ".join(f"{k} {rw.blind_share(c['g64'][k], c['vis'], c['P']):.0%} / {rw.blind_share(c['g64'][k], c['vis'], c['P'], 1e-2):.0%}"
                                             for k in rw.GRADS if c["g64"][k].size))
        for path in PATHS:
            r = run_path(name, path, o32, o64)
            lines.append(rw.format_table(r["cmp"], f"{name} {path}: fp32 oracle | HIP, both against the fp64 oracle"))
            if "cmp32" in r:
                lines.append(f"# n_contrib differs from the fp32 oracle's in {r['n_contrib_mismatch']} pixels")
                lines.append(rw.format_table(r["cmp32"], f"{name} {path}: HIP against the fp32 oracle directly (informative; ratios are to the 4-ulp floor)"))
            quant = ("median", "p90") if r["strict"] else ("median",)
            for label, (ratio, s, q) in rw.max_ratio(r["cmp"], quant).items():
                key = (path.split("-")[1], label.split(".")[0])
                if ratio > top.get(key, (0.0,))[0]:
                    top[key] = (ratio, f"{name} {path} {label} stratum 1e-{s} {q}")
            print(lines[-1] if "cmp32" not in r else lines[-3], flush=True)
    lines.append("## largest judged ratio HIP error / max(fp32-oracle error, 4 * 2^-23) per arithmetic and tensor (strict: median and p90; fast: median)")
    for (mode, label), (ratio, where) in sorted(top.items()):
        lines.append(f"{mode:<7} {label:<12} {ratio:6.2f}   {where}")
    for mode in ("strict", "fast"):
        lines.append(f"{mode}: maximum {max(v[0] for k, v in top.items() if k[0] == mode):.2f}")
    text = "\n".join(lines) + "\n"
    print("\n".join(lines[-len(top) - 3:]))
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
