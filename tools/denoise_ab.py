"""The denoiser against uniform sampling (include/jade_bvh.h: jade_render_guides, jade_render_denoise, jade_denoise_image).

usage: python tools/denoise_ab.py [--setups C2,C3] [--out profiles/denoise_ab.json]

Per setup (tools/adaptive_ab.py's: C2 at 512^2, C3 at 1080p, early-exit walk): uniform renders at 16 / 64 / 256 / 1024 spp, each
compared raw and denoised with jade_denoise_defaults against a uniform 8192-spp reference of frame 1 << 20 (samples disjoint from
every compared render's), with adaptive_ab.py's relMSE.  Per render: kernel ms of the render (jade_stats.kernel_ms), wall ms of
jade_render_guides (guides and variance), of jade_denoise_image (the filter alone, with its copies) and of jade_render_denoise (all of
it on the device, one copy back); the calls are synchronous.  "equivalent_spp": the uniform spp whose relMSE a denoised frame
reaches, interpolated in log-log between the measured uniform points (None above the range).  "sweep": relMSE of the 64-spp frame
filtered with other parameters around the defaults (jade_denoise_image on the same inputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B  # noqa: E402

from adaptive_ab import REF_FRAME, SETUPS, rel_mse  # noqa: E402

REF_SPP = 8192
SPPS = (16, 64, 256, 1024)


def equivalent_spp(err, uniform):
    """uniform: {spp: relMSE}; the spp at which the uniform curve reaches err (log-log interpolation; None past the last point)."""
    pts = sorted((int(k), v) for k, v in uniform.items())
    if err >= pts[0][1]:
        return float(pts[0][0]) * pts[0][1] / err  # (below the range: relMSE ~ 1 / spp)
    for (s0, e0), (s1, e1) in zip(pts, pts[1:]):
        if e1 <= err <= e0:
            f = (np.log(err) - np.log(e0)) / (np.log(e1) - np.log(e0))
            return float(np.exp(np.log(s0) + f * (np.log(s1) - np.log(s0))))
    return None


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def run(name, s):
    hs, cfg = J.build_config(s["config"])
    p = B.params_from_config(cfg, spp=s["cap"], walk=_abi.WALK_EARLY_EXIT)
    p.width, p.height = s["width"], s["height"]
    hip = J.hip()
    d = hip.denoise_defaults()
    defaults = {k: getattr(d, k) for k, _ in _abi.DenoiseParams._fields_}
    res = dict(setup=dict(config=s["config"], width=p.width, height=p.height, walk="early_exit", ref_spp=REF_SPP, ref_frame=REF_FRAME),
               defaults=defaults, uniform={}, denoised={}, sweep={})
    with hip.scene(hs) as sc:
        q = type(p).from_buffer_copy(p)
        q.spp, q.frame = REF_SPP, REF_FRAME
        ref, res["reference_wall_ms"] = timed(lambda: sc.render(q, want_bgr8=False)[0])
        for spp in SPPS:
            q = type(p).from_buffer_copy(p)
            q.spp = spp
            sc.begin(q)
            st = sc.step(spp)
            sc.flush(st)
            rgb, _ = sc.resolve(want_bgr8=False)
            sc.guides(d.guide_spp)  # warm-up: first use allocates the denoiser's buffers
            g, guide_ms = timed(lambda: sc.guides(d.guide_spp))
            den_img, filter_ms = timed(lambda: hip.denoise_image(rgb, g["variance"], g["albedo"], g["normal"], g["depth"], params=d))
            (den, _), denoise_ms = timed(lambda: sc.denoise(d, want_bgr8=False))
            assert np.array_equal(den.view(np.uint32), den_img.view(np.uint32))
            res["uniform"][str(spp)] = dict(rel_mse=rel_mse(rgb, ref), kernel_ms=st.kernel_ms, rays=int(st.rays))
            res["denoised"][str(spp)] = dict(rel_mse=rel_mse(den, ref), guides_wall_ms=guide_ms, filter_wall_ms=filter_ms,
                                             denoise_wall_ms=denoise_ms)
            print(name, spp, json.dumps(res["uniform"][str(spp)]), json.dumps(res["denoised"][str(spp)]), flush=True)
            if spp == 64:
                for it in (3, 5):
                    for sl in (2.0, 4.0, 8.0):
                        for sn in (32.0, 128.0):
                            dd = hip.denoise_defaults()
                            dd.iterations, dd.sigma_luminance, dd.sigma_normal = it, sl, sn
                            x = hip.denoise_image(rgb, g["variance"], g["albedo"], g["normal"], g["depth"], params=dd)
                            res["sweep"][f"it{it}_sl{sl:g}_sn{sn:g}"] = rel_mse(x, ref)
        uni = {k: v["rel_mse"] for k, v in res["uniform"].items()}
        for v in res["denoised"].values():
            v["equivalent_spp"] = equivalent_spp(v["rel_mse"], uni)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setups", default="C2,C3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_ab.json"))
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
