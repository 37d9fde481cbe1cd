"""JADE_ENV_MIXTURE (include/jade_rt.h) against JADE_ENV_REFERENCE and JADE_ENV_IMPORTANCE, under uniform and cosine bounces: what DESIGN.md 3.16 quotes.

usage: python tools/env_mixture_ab.py [--out profiles/env_mixture_ab.json] [--scenes ball,C2,C3] [--repeats 3] [--step-spp 64] [--converged-spp 2048] [--frames 6]
           The sky-lit ball (a diffuse ball and slab under the procedural 64 x 32 sky, 48 x 40) and the built-in configurations at their
           own sizes, with the early-exit walk, the modes alternating in ONE scene handle, under each bounce sampling:
             time     one step of --step-spp samples plus flush, --repeats times per mode after a warm-up each: device time per sample
                      from jade_stats
             noise    at EQUAL samples per pixel, 16 / 64 / 256, --frames independent frames per mode and count, against the mean of the
                      modes' converged frames of --converged-spp samples each:
                      relMSE = mean over the compared pixels and channels of e = (x - ref)^2 / (ref^2 + 1e-4), and the MEDIAN over the
                      compared pixels of e's mean over the channels - a figure rare bright samples do not carry (relMSE
                      alone resolves nothing on C2 and C3).
                      Sky pixels are left out: a pixel whose converged frames are all the same bits reached no sampling vertex.
           No threshold: the figures are reported as measured, the cases where the mixture loses included.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B, host as H  # noqa: E402

BOUNCES = (("uniform", _abi.BOUNCE_UNIFORM), ("cosine", _abi.BOUNCE_COSINE))
ENVS = (("reference", _abi.ENV_REFERENCE), ("importance", _abi.ENV_IMPORTANCE), ("mixture", _abi.ENV_MIXTURE))
NOISE_SPP = (16, 64, 256)


def sky_lit_ball():
    cfg = J.SceneBuilder().config("tiny")  # (the camera only)
    b = J.SceneBuilder()
    b.add_proc("geodesic", 3, H.material(brdf=(0.6, 0.55, 0.5)), H.transform_matrix(trans=(0.1, -1.2, 1.0), scale=(1.1, 1.1, 1.1)))
    b.add_proc("box", 0, H.material(brdf=(0.5, 0.5, 0.5)), H.transform_matrix(trans=(0.0, -2.3, 1.0), scale=(9.0, 0.2, 9.0)))
    b.set_env_sky(64, 32)
    return b.build(), cfg, (48, 40)


def params(cfg, size, spp, env, frame=0):
    p = B.params_from_config(cfg)
    if size:
        p.width, p.height = size
    p.spp, p.frame, p.env_sampling, p.walk = spp, frame, env, _abi.WALK_EARLY_EXIT
    return p


def timed(sc, p):
    st = _abi.Stats()
    sc.begin(p)
    sc.step(p.spp, st)
    sc.flush(st)
    return dict(kernel_ms=st.kernel_ms, ms_per_sample=st.kernel_ms / p.spp, rays=st.rays, rays_env=st.rays_env, mray_per_s=st.rays / st.kernel_ms / 1e3)


def alternate(sc, make, repeats):
    runs = {name: [] for name, _ in ENVS}
    for k in range(repeats + 1):
        for name, env in ENVS:
            r = timed(sc, make(env))
            if k:
                runs[name].append(r)
    return {name: dict(runs=rs, ms_per_sample_median=float(np.median([r["ms_per_sample"] for r in rs]))) for name, rs in runs.items()}


def errors(x, ref, keep):
    """(relMSE, the median over the pixels of the relative squared error)"""
    x, ref = x.astype(np.float64)[keep], ref.astype(np.float64)[keep]
    e = (x - ref) ** 2 / (ref ** 2 + 1e-4)
    return float(e.mean()), float(np.median(e.mean(-1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_mixture_ab.json"))
    ap.add_argument("--scenes", default="ball,C2,C3")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-spp", type=int, default=64)
    ap.add_argument("--converged-spp", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=6)
    a = ap.parse_args()
    hip = J.hip()
    res = {"what": __doc__.strip().splitlines()[0], "repeats": a.repeats, "step_spp": a.step_spp, "converged_spp_per_mode": a.converged_spp,
           "frames": a.frames, "scenes": {}}
    if os.path.exists(a.out):  # (scenes measured by an earlier call, and the kernel comparison's runs in the same file, stay)
        with open(a.out) as fi:
            old = json.load(fi)
        res = dict(old, **res, scenes=old.get("scenes", {}))
    for name in a.scenes.split(","):
        hs, cfg, size = sky_lit_ball() if name == "ball" else J.build_config(name) + (None,)
        p0 = params(cfg, size, 1, 0)
        out = {"width": int(p0.width), "height": int(p0.height), "triangles": int(hs.n_triangles), "emitter_entries": int(len(hs.a["emit"]))}
        with hip.scene(hs) as sc:
            for bounce_name, bounce in BOUNCES:
                sc.set_bounce_sampling(bounce)
                e = {"time": dict(spp=a.step_spp, **alternate(sc, lambda env: params(cfg, size, a.step_spp, env), a.repeats))}
                conv = {n: sc.render(params(cfg, size, a.converged_spp, env, frame=900000), want_bgr8=False)[0] for n, env in ENVS}
                ref = np.mean([c.astype(np.float64) for c in conv.values()], 0)
                same = np.ones(ref.shape[:2], bool)
                for c in conv.values():
                    same &= (c.view(np.uint32) == conv["reference"].view(np.uint32)).all(-1)
                keep = ~same
                e["compared_pixels"] = int(keep.sum())
                e["converged_total_over_reference"] = {n: float(c.astype(np.float64)[keep].sum() / conv["reference"].astype(np.float64)[keep].sum())
                                                       for n, c in conv.items()}
                e["noise"] = {}
                for spp in NOISE_SPP:
                    row = {}
                    for n, env in ENVS:
                        v = [errors(sc.render(params(cfg, size, spp, env, frame=1000 * k), want_bgr8=False)[0], ref, keep) for k in range(1, a.frames + 1)]
                        row[n] = dict(rel_mse=[x[0] for x in v], rel_mse_mean=float(np.mean([x[0] for x in v])),
                                      median_rel_sq_err=[x[1] for x in v], median_rel_sq_err_mean=float(np.mean([x[1] for x in v])))
                    for n in ("importance", "mixture"):
                        row[f"rel_mse_{n}_over_reference"] = row[n]["rel_mse_mean"] / row["reference"]["rel_mse_mean"]
                        row[f"median_{n}_over_reference"] = row[n]["median_rel_sq_err_mean"] / row["reference"]["median_rel_sq_err_mean"]
                    e["noise"][str(spp)] = row
                out[bounce_name] = e
                t = e["time"]
                print(f"{name} bounce {bounce_name}: ms per sample " + " ".join(f"{n} {t[n]['ms_per_sample_median']:.4f}" for n, _ in ENVS) + "; " +
                      "; ".join(f"{s} spp relMSE imp/ref {e['noise'][str(s)]['rel_mse_importance_over_reference']:.3f} mix/ref "
                                f"{e['noise'][str(s)]['rel_mse_mixture_over_reference']:.3f} median imp/ref {e['noise'][str(s)]['median_importance_over_reference']:.3f} "
                                f"mix/ref {e['noise'][str(s)]['median_mixture_over_reference']:.3f}" for s in NOISE_SPP) +
                      f"; converged totals over reference {e['converged_total_over_reference']} over {e['compared_pixels']} pixels", flush=True)
            sc.set_bounce_sampling(_abi.BOUNCE_UNIFORM)
        res["scenes"][name] = out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
