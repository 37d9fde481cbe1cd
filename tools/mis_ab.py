"""Multiple importance sampling of the emitters (include/jade_bvh.h: jade_scene_set_direct_sampling) against the emitter rays alone, both under cosine-weighted bounces: what DESIGN.md 3.13 quotes.

usage: python tools/mis_ab.py [--out profiles/mis_ab.json] [--scenes C2,C3,contact,lamp] [--repeats 3] [--step-spp 64] [--converged-spp 2048] [--frames 6]
           C2 and C3 at their own sizes, the contact scene (tests/mis_cases.py: a lamp quad standing on a floor) and the 84-entry lamp
           scene (tests/lamp_scenes.py) at 192 x 160; the two modes alternating in ONE scene handle, JADE_BOUNCE_COSINE set throughout:
             time     C2 and C3: one step of --step-spp samples plus flush, --repeats times per mode after a warm-up each: device time
                      per sample from jade_stats.  The rays are the same rays, so level is expected; the runs are written down.
             noise    relMSE at EQUAL samples per pixel, 16 / 64 / 256, --frames independent frames per mode and count, against the mean
                      of two converged frames, one per mode, of --converged-spp samples each:
                      relMSE = mean over the compared pixels and channels of (x - ref)^2 / (ref^2 + 1e-4);
                      every single frame's figure is kept, with the largest over the smallest of a mode's frames (the spread), and
                      `outliers`: the pixel channels of a frame above 8 x (ref + 0.05) - the rare bright samples themselves.
                      Pixels whose two converged frames are the same bits (open sky, an emitter seen directly) are left out.
           No threshold: the figures are reported as measured.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import _abi, backend as B  # noqa: E402

MODES = (("rays", _abi.DIRECT_RAYS), ("mis", _abi.DIRECT_MIS))
NOISE_SPP = (16, 64, 256)
SMALL_W, SMALL_H = 192, 160


def scene_of(name):
    """(host scene, params(spp, frame), timed?)"""
    if name in ("contact", "lamp"):
        if name == "contact":
            import mis_cases
            hs = mis_cases.contact()
            eye, cam = mis_cases.contact_camera()
        else:
            import lamp_scenes
            from jaderaytracerendering_amd import host as H
            hs = lamp_scenes.lamp_scene("lamp")
            eye, cam = H.camera_orbit(5.0, 20.0, 30.0)
        return hs, (lambda spp, frame=0: B.make_params(SMALL_W, SMALL_H, spp, eye, cam, frame=frame, walk=_abi.WALK_EARLY_EXIT)), False
    hs, cfg = J.build_config(name)

    def make(spp, frame=0):
        p = B.params_from_config(cfg)
        p.spp, p.frame, p.walk = spp, frame, _abi.WALK_EARLY_EXIT
        return p
    return hs, make, True


def timed(sc, mode, p):
    sc.set_direct_sampling(mode)
    st = _abi.Stats()
    sc.begin(p)
    sc.step(p.spp, st)
    sc.flush(st)
    return dict(kernel_ms=st.kernel_ms, ms_per_sample=st.kernel_ms / p.spp, rays=st.rays, rays_shadow=st.rays_shadow, rays_indirect=st.rays_indirect,
                nodes_visited=st.nodes_visited, mray_per_s=st.rays / st.kernel_ms / 1e3)


def alternate(sc, p, repeats):
    runs = {name: [] for name, _ in MODES}
    for k in range(repeats + 1):
        for name, mode in MODES:
            r = timed(sc, mode, p)
            if k:
                runs[name].append(r)
    return {name: dict(runs=rs, ms_per_sample_median=float(np.median([r["ms_per_sample"] for r in rs]))) for name, rs in runs.items()}


def rel_mse(x, ref, keep):
    x, ref = x.astype(np.float64)[keep], ref.astype(np.float64)[keep]
    return float(((x - ref) ** 2 / (ref ** 2 + 1e-4)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mis_ab.json"))
    ap.add_argument("--scenes", default="C2,C3,contact,lamp")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-spp", type=int, default=64)
    ap.add_argument("--converged-spp", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=6)
    a = ap.parse_args()
    hip = J.hip()
    res = {"what": __doc__.strip().splitlines()[0], "repeats": a.repeats, "converged_spp_per_mode": a.converged_spp, "frames": a.frames, "scenes": {}}
    for name in a.scenes.split(","):
        hs, make, is_timed = scene_of(name)
        p0 = make(1)
        e = {"width": int(p0.width), "height": int(p0.height), "triangles": int(hs.n_triangles), "emitter_entries": int(len(hs.a["emit"]))}
        with hip.scene(hs) as sc:
            sc.set_bounce_sampling(_abi.BOUNCE_COSINE)
            if is_timed:
                e["time"] = dict(spp=a.step_spp, **alternate(sc, make(a.step_spp), a.repeats))
            conv = {}
            for mode_name, mode in MODES:
                sc.set_direct_sampling(mode)
                conv[mode_name] = sc.render(make(a.converged_spp, frame=900000), want_bgr8=False)[0]
            ref = 0.5 * (conv["rays"].astype(np.float64) + conv["mis"].astype(np.float64))
            keep = ~(conv["rays"].view(np.uint32) == conv["mis"].view(np.uint32)).all(-1)
            e["compared_pixels"] = int(keep.sum())
            e["converged_frames_rel_difference"] = rel_mse(conv["mis"], conv["rays"], keep)
            e["converged_total_mis_over_rays"] = float(conv["mis"].astype(np.float64)[keep].sum() / conv["rays"].astype(np.float64)[keep].sum())
            e["noise"] = {}
            for spp in NOISE_SPP:
                row = {}
                for mode_name, mode in MODES:
                    sc.set_direct_sampling(mode)
                    v, o, mx = [], [], []
                    for k in range(1, a.frames + 1):
                        x = sc.render(make(spp, frame=1000 * k), want_bgr8=False)[0]
                        v.append(rel_mse(x, ref, keep))
                        o.append(int((x.astype(np.float64)[keep] > 8 * (ref[keep] + 0.05)).sum()))
                        mx.append(float((x.astype(np.float64)[keep] / (ref[keep] + 0.05)).max()))
                    row[mode_name] = dict(rel_mse=v, rel_mse_mean=float(np.mean(v)), rel_mse_median=float(np.median(v)),
                                          spread_max_over_min=float(max(v) / min(v)), outliers=o, largest_sample_over_ref=mx)
                row["rel_mse_mis_over_rays"] = row["mis"]["rel_mse_mean"] / row["rays"]["rel_mse_mean"]
                row["rel_mse_median_mis_over_rays"] = row["mis"]["rel_mse_median"] / row["rays"]["rel_mse_median"]
                e["noise"][str(spp)] = row
        res["scenes"][name] = e
        t = e.get("time")
        print(f"{name}: " + (f"ms per sample rays {t['rays']['ms_per_sample_median']:.3f} mis {t['mis']['ms_per_sample_median']:.3f}; " if t else "") +
              "relMSE mis / rays (spread rays, mis; outliers rays, mis) at " +
              ", ".join(f"{s} spp {e['noise'][str(s)]['rel_mse_mis_over_rays']:.3f} ({e['noise'][str(s)]['rays']['spread_max_over_min']:.1f}, "
                        f"{e['noise'][str(s)]['mis']['spread_max_over_min']:.1f}; {sum(e['noise'][str(s)]['rays']['outliers'])}, {sum(e['noise'][str(s)]['mis']['outliers'])})"
                        for s in NOISE_SPP) +
              f"; converged totals mis / rays {e['converged_total_mis_over_rays']:.5f} over {e['compared_pixels']} pixels", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
