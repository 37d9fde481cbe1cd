"""Smooth shading (include/jade_bvh.h: jade_scene_set_vertex_normals) against the flat render: what DESIGN.md 3.19 quotes.

usage: python tools/smooth_ab.py [--out profiles/smooth_ab.json] [--configs C2,C3] [--frames 16] [--spp 64] [--converged-spp 4096] [--crease 60]
           C2 at 512 x 512 and C3 at 1920 x 1080, every object of the configuration smoothed at --crease degrees.
             cost     --frames frames of --spp samples each, device time from jade_stats, three renders alternating frame by frame: the
                      smooth render (it runs the list schedule), the flat render under the same list schedule (JADE_FUSED=0 JADE_TAIL=0,
                      read when the handle is made) and the flat render under the default schedule.  Both ratios are written down: the
                      second includes the price of losing the fused first pass and is what a user pays.
             denoise  per mode: relMSE of the denoised --spp frame against a --converged-spp render of the SAME mode,
                      mean over pixels and channels of (x - ref)^2 / (ref^2 + 1e-4), over the whole frame and over the smoothed pixels
                      (those whose normal guide differs between the two modes); and the share of the smoothed pixels at which the
                      filter's normal weight, max(dot(n, n'), 0)^sigma_normal of the guide normals, is below 1/2 towards one of the four
                      neighbours - the filter cuts that neighbour.
           No threshold: the figures are reported as measured.
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

SIZES = {"C2": (512, 512), "C3": (1920, 1080)}
LIST = {"JADE_FUSED": "0", "JADE_TAIL": "0"}


def build(name, crease):
    b = H.SceneBuilder()
    try:
        b.set_smoothing(crease)
        cfg = b.config(name)
        return b.build(), cfg
    finally:
        b.close()


def scene_under(hip, hs, env):
    """A handle made with `env` in the environment (the switches are read once, at jade_scene_create)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return hip.scene(hs)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def params(cfg, size, spp, frame):
    p = B.params_from_config(cfg)
    p.width, p.height = size
    p.spp, p.frame, p.walk = spp, frame, _abi.WALK_EARLY_EXIT
    return p


def rel_mse(x, ref, keep=None):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    e = (x - ref) ** 2 / (ref ** 2 + 1e-4)
    return float(e.mean() if keep is None else e[keep].mean())


def cut_share(normal, keep, sigma):
    n = normal.astype(np.float64)
    cut = np.zeros(n.shape[:2], bool)
    for axis, shift in ((0, 1), (0, -1), (1, 1), (1, -1)):
        d = np.maximum((n * np.roll(n, shift, axis)).sum(-1), 0.0) ** sigma
        edge = np.zeros_like(cut)
        idx = [slice(None)] * 2
        idx[axis] = 0 if shift == 1 else -1
        edge[tuple(idx)] = True                     # (the rolled-in row is no neighbour)
        cut |= (d < 0.5) & ~edge
    return float(cut[keep].mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_ab.json"))
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--converged-spp", type=int, default=4096)
    ap.add_argument("--crease", type=float, default=60.0)
    a = ap.parse_args()
    hip = J.hip()
    res = {"what": __doc__.strip().splitlines()[0], "frames": a.frames, "spp": a.spp, "converged_spp": a.converged_spp, "crease_deg": a.crease, "configs": {}}
    for name in a.configs.split(","):
        size = SIZES[name]
        hs, cfg = build(name, a.crease)
        vn = hs.vertex_normals
        hs.vertex_normals = None
        flat_rows = (np.abs(vn - hs.tri_f32()[:, None, 10:13]).max((1, 2)) == 0).sum()
        out = {"width": size[0], "height": size[1], "triangles": int(hs.n_triangles), "flat_triangles_in_the_table": int(flat_rows)}
        with scene_under(hip, hs, {}) as flat_default, scene_under(hip, hs, LIST) as flat_list, scene_under(hip, hs, {}) as smooth:
            smooth.set_vertex_normals(vn)
            runs = {"smooth": (smooth, []), "flat_list": (flat_list, []), "flat_default": (flat_default, [])}
            for frame in range(a.frames + 1):            # frame 0 warms up
                for key, (sc, ms) in runs.items():
                    st = sc.render(params(cfg, size, a.spp, 1000 * frame), want_rgb=False, want_bgr8=False)[2]
                    if frame:
                        ms.append(dict(kernel_ms=st.kernel_ms, rays=st.rays, rays_inline=st.rays_inline, tail_launches=st.tail_launches))
            cost = {k: dict(frames=ms, kernel_ms_total=float(sum(m["kernel_ms"] for m in ms)), rays_total=int(sum(m["rays"] for m in ms))) for k, (_, ms) in runs.items()}
            cost["smooth_over_flat_list"] = cost["smooth"]["kernel_ms_total"] / cost["flat_list"]["kernel_ms_total"]
            cost["smooth_over_flat_default"] = cost["smooth"]["kernel_ms_total"] / cost["flat_default"]["kernel_ms_total"]
            out["cost"] = cost
            dn = {}
            sigma = hip.denoise_defaults().sigma_normal
            guides = {}
            for key, sc in (("smooth", smooth), ("flat", flat_default)):
                ref = sc.render(params(cfg, size, a.converged_spp, 900000), want_bgr8=False)[0]
                sc.render(params(cfg, size, a.spp, 5000), want_rgb=False, want_bgr8=False)
                guides[key] = sc.guides()["normal"]
                dn[key] = dict(ref=ref, den=sc.denoise(want_bgr8=False)[0], raw=sc.resolve(want_bgr8=False)[0])
            keep = (guides["smooth"] != guides["flat"]).any(-1)
            out["denoise"] = {"smoothed_pixels": int(keep.sum()), "sigma_normal": float(sigma)}
            for key in ("smooth", "flat"):
                d = dn[key]
                out["denoise"][key] = dict(rel_mse_denoised=rel_mse(d["den"], d["ref"]), rel_mse_denoised_smoothed_pixels=rel_mse(d["den"], d["ref"], keep),
                                           rel_mse_raw=rel_mse(d["raw"], d["ref"]), rel_mse_raw_smoothed_pixels=rel_mse(d["raw"], d["ref"], keep),
                                           normal_cut_share_smoothed_pixels=cut_share(guides[key], keep, sigma))
        res["configs"][name] = out
        c, d = out["cost"], out["denoise"]
        print(f"{name}: smooth / flat (list schedule) {c['smooth_over_flat_list']:.3f}, smooth / flat (default schedule) {c['smooth_over_flat_default']:.3f}; "
              f"denoised relMSE on {d['smoothed_pixels']} smoothed pixels: smooth {d['smooth']['rel_mse_denoised_smoothed_pixels']:.4g} flat "
              f"{d['flat']['rel_mse_denoised_smoothed_pixels']:.4g}; cut share smooth {d['smooth']['normal_cut_share_smoothed_pixels']:.3f} flat "
              f"{d['flat']['normal_cut_share_smoothed_pixels']:.3f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
