"""Adaptive sampling against uniform sampling at equal error (include/jade_bvh.h, jade_render_adaptive).

usage: python tools/adaptive_ab.py [--setups C2,C3] [--out profiles/adaptive_ab.json]

Per setup: uniform renders at 256 / 512 / 1024 spp and adaptive renders (cap 1024) at two rel_error values, each compared with a
uniform 8192-spp reference rendered with frame = 1 << 20, so that its samples are disjoint from every compared render's (sample s
draws the stream of frame + s, jade_rt.h).  Error figure:

    relMSE = mean over pixels and channels of (x - r)^2 / (r^2 + 1e-2)

(x: the render's linear radiance, r: the reference's; the 1e-2 keeps black pixels from dominating).  The reference has noise of its
own, so relMSE has a floor of about 1/8 of a 1024-spp render's own.  The two rel_error values come from the data: the median tile
error of the uniform 256- and 1024-spp renders (tile error = max over the tile's pixels of jade_render_error), so that about half
the tiles converge by 256 and by 1024 samples.  Per render: kernel ms (jade_stats.kernel_ms), wall ms of the call, rays, samples,
host waits, the histogram of tile sample counts.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B  # noqa: E402

from adaptive_ref import tile_errors  # noqa: E402

SETUPS = {
    "C2": dict(config="C2", width=512, height=512, cap=1024, min_spp=32),
    "C3": dict(config="C3", width=1920, height=1080, cap=1024, min_spp=16),
}
FLOOR = 0.01
REF_SPP = 8192
REF_FRAME = 1 << 20


def rel_mse(x, r):
    x = x.astype(np.float64)
    r = r.astype(np.float64)
    return float(np.mean((x - r) ** 2 / (r * r + 1e-2)))


def record(st, wall_ms, x, ref, tile_spp=None):
    out = dict(kernel_ms=st.kernel_ms, wall_ms=wall_ms, rays=int(st.rays), samples=int(st.samples), host_syncs=int(st.host_syncs),
               mray_per_s=st.rays / st.kernel_ms / 1e3 if st.kernel_ms > 0 else None, rel_mse=rel_mse(x, ref))
    if tile_spp is not None:
        ks, n = np.unique(tile_spp, return_counts=True)
        out["tile_spp"] = {str(int(k)): int(c) for k, c in zip(ks, n)}
    return out


def run(name, s):
    hs, cfg = J.build_config(s["config"])
    p = B.params_from_config(cfg, spp=s["cap"], walk=_abi.WALK_EARLY_EXIT)
    p.width, p.height = s["width"], s["height"]
    tx, ty = (p.width + 15) // 16, (p.height + 15) // 16
    res = dict(setup=dict(s, walk="early_exit", error_floor=FLOOR, ref_spp=REF_SPP, ref_frame=REF_FRAME), uniform={}, adaptive={})
    with J.hip().scene(hs) as sc:
        q = type(p).from_buffer_copy(p)
        q.spp, q.frame = REF_SPP, REF_FRAME
        t0 = time.perf_counter()
        ref = sc.render(q, want_bgr8=False)[0]
        res["reference_wall_ms"] = (time.perf_counter() - t0) * 1e3
        sc.render(type(p).from_buffer_copy(p), want_bgr8=False)  # warm-up at the cap
        medians = {}
        for spp in (256, 512, 1024):
            q = type(p).from_buffer_copy(p)
            q.spp = spp
            t0 = time.perf_counter()
            rgb, _, st = sc.render(q, want_bgr8=False)
            wall = (time.perf_counter() - t0) * 1e3
            res["uniform"][str(spp)] = record(st, wall, rgb, ref, np.full((ty, tx), spp))
            if spp in (256, 1024):
                medians[spp] = float(np.median(tile_errors(sc.error_map(FLOOR), tx, ty)))
            print(name, "uniform", spp, json.dumps(res["uniform"][str(spp)]), flush=True)
        res["tile_error_median"] = {str(k): v for k, v in medians.items()}
        for spp in (256, 1024):
            rel = medians[spp]
            t0 = time.perf_counter()
            rgb, _, tspp, st = sc.render_adaptive(p, s["min_spp"], rel, FLOOR, want_bgr8=False)
            wall = (time.perf_counter() - t0) * 1e3
            r = record(st, wall, rgb, ref, tspp)
            r["rel_error"] = rel
            res["adaptive"][f"{rel:.6g}"] = r
            print(name, "adaptive", rel, json.dumps(r), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setups", default="C2,C3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_ab.json"))
    a = ap.parse_args()
    out = {"what": __doc__.strip().splitlines()[0], "relmse": "mean over pixels and channels of (x - r)^2 / (r^2 + 1e-2)", "setups": {}}
    for name in a.setups.split(","):
        out["setups"][name] = run(name, SETUPS[name])
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
