"""Normal maps (include/jade_bvh.h: jade_scene_set_normal_maps) against the same textured scene without them: what DESIGN.md 3.21 quotes.

usage: python tools/normal_map_ab.py [--out profiles/normal_map_ab.json] [--configs C2,C3] [--frames 16] [--spp 64] [--converged-spp 4096]
           C2 at 512 x 512 and C3 at 1920 x 1080, textured as tools/texture_ab.py textures them.  The floor (object 2, planar UVs from
           above) and the statue (object 0, spherical UVs) carry the host.height_to_normal_map of a lattice of bumps - 1024 x 1024 texels,
           64 x 64 bumps on the floor, 32 x 32 on the statue, steepest slope 0.5.
             cost     --frames frames of --spp samples each after a warm-up frame, device time from jade_stats, two renders alternating
                      frame by frame: the mapped render and the same textured scene without the map - both run the list schedule, so the
                      ratio is the map's own price.  Per sample and per ray, and the ray counts of both: a map changes rays through the
                      culls against the flat normal, and by how much is written down.
             denoise  relMSE of the denoised --spp frame of the MAPPED scene against a --converged-spp render of it, mean over pixels and
                      channels of (x - ref)^2 / (ref^2 + 1e-4): with the mapped render's own normal guide (jade_render_denoise), and with
                      the unmapped scene's normal guide in its place (jade_denoise_image on the same frame, variance, albedo and depth).
           No threshold: the figures are reported as measured.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import jaderaytracerendering_amd as J  # noqa: E402
from jaderaytracerendering_amd import host as H  # noqa: E402
from texture_ab import CHECKER, FLOOR, SIZES, SQUARES, STATUE, params, rel_mse, scene_under, statue_image  # noqa: E402

MAP_SIZE = 1024


def bumps(n, size=MAP_SIZE):
    """host.height_to_normal_map of n x n bumps on size x size texels: height = (0.08 / n) sin(2 pi n u) sin(2 pi n v) at the texel centres."""
    c = (np.arange(size) + 0.5) / size
    h = (0.08 / n) * np.sin(2 * np.pi * n * c)[None, :] * np.sin(2 * np.pi * n * c)[:, None]
    return H.height_to_normal_map(h.astype(np.float32), 1.0)


def build(name, mapped):
    b = H.SceneBuilder()
    try:
        b.set_object_texture(STATUE, statue_image(), H.UV_SPHERICAL)
        b.set_object_texture(FLOOR, H.texture_checker(CHECKER, SQUARES, (0.9, 0.9, 0.9), (0.15, 0.15, 0.15)), H.UV_PLANAR_Y)
        if mapped:
            b.set_object_normal_map(STATUE, bumps(32), H.UV_SPHERICAL, 1.0)
            b.set_object_normal_map(FLOOR, bumps(64), H.UV_PLANAR_Y, 1.0)
        cfg = b.config(name)
        return b.build(), cfg
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_map_ab.json"))
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--converged-spp", type=int, default=4096)
    a = ap.parse_args()
    hip = J.hip()
    res = {"what": __doc__.strip().splitlines()[0], "frames": a.frames, "spp": a.spp, "converged_spp": a.converged_spp,
           "map": [MAP_SIZE, {"floor_bumps": 64, "statue_bumps": 32}], "configs": {}}
    for name in a.configs.split(","):
        size = SIZES[name]
        hs, cfg = build(name, True)
        plain_hs, _ = build(name, False)
        assert np.array_equal(hs.a["triangles"], plain_hs.a["triangles"]) and plain_hs.normal_maps is None
        out = {"width": size[0], "height": size[1], "triangles": int(hs.n_triangles), "mapped_triangles": int((hs.normal_maps[2] >= 0).sum())}
        with scene_under(hip, plain_hs, {}) as plain, scene_under(hip, hs, {}) as mapped:
            runs = {"mapped": (mapped, []), "unmapped": (plain, [])}
            for frame in range(a.frames + 1):            # frame 0 warms up
                for key, (sc, ms) in runs.items():
                    st = sc.render(params(cfg, size, a.spp, 1000 * frame), want_rgb=False, want_bgr8=False)[2]
                    if frame:
                        ms.append(dict(kernel_ms=st.kernel_ms, rays=st.rays, samples=st.samples, rays_inline=st.rays_inline, tail_launches=st.tail_launches))
            cost = {}
            for k, (_, ms) in runs.items():
                total, rays, samples = float(sum(m["kernel_ms"] for m in ms)), int(sum(m["rays"] for m in ms)), int(sum(m["samples"] for m in ms))
                cost[k] = dict(frames=ms, kernel_ms_total=total, rays_total=rays, samples_total=samples, ns_per_ray=1e6 * total / rays, ns_per_sample=1e6 * total / samples)
            cost["mapped_over_unmapped"] = cost["mapped"]["kernel_ms_total"] / cost["unmapped"]["kernel_ms_total"]
            cost["mapped_over_unmapped_per_ray"] = cost["mapped"]["ns_per_ray"] / cost["unmapped"]["ns_per_ray"]
            cost["rays_mapped_over_unmapped"] = cost["mapped"]["rays_total"] / cost["unmapped"]["rays_total"]
            out["cost"] = cost
            ref = mapped.render(params(cfg, size, a.converged_spp, 900000), want_bgr8=False)[0]
            p = params(cfg, size, a.spp, 5000)
            plain.render(p, want_rgb=False, want_bgr8=False)
            plain_normal = plain.guides()["normal"]
            raw = mapped.render(p, want_bgr8=False)[0]
            g = mapped.guides()
            den_own = mapped.denoise(want_bgr8=False)[0]
            den_same = hip.denoise_image(raw, g["variance"], g["albedo"], g["normal"], g["depth"])       # the same filter through the image entry
            den_plain = hip.denoise_image(raw, g["variance"], g["albedo"], plain_normal, g["depth"])
            out["denoise"] = dict(image_entry_equals_render_entry=bool(np.array_equal(den_own.view(np.uint32), den_same.view(np.uint32))),
                                  rel_mse_raw=rel_mse(raw, ref), rel_mse_mapped_guide=rel_mse(den_own, ref), rel_mse_unmapped_guide=rel_mse(den_plain, ref))
        res["configs"][name] = out
        c, d = out["cost"], out["denoise"]
        print(f"{name}: mapped / unmapped time {c['mapped_over_unmapped']:.3f}, per ray {c['mapped_over_unmapped_per_ray']:.3f} "
              f"(ns per ray {c['mapped']['ns_per_ray']:.4f} / {c['unmapped']['ns_per_ray']:.4f}, ns per sample {c['mapped']['ns_per_sample']:.3f} / "
              f"{c['unmapped']['ns_per_sample']:.3f}); rays mapped / unmapped {c['rays_mapped_over_unmapped']:.4f}; denoised relMSE: mapped guide "
              f"{d['rel_mse_mapped_guide']:.4g}, unmapped guide {d['rel_mse_unmapped_guide']:.4g}, raw {d['rel_mse_raw']:.4g}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
