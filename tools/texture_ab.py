"""Albedo textures (include/jade_bvh.h: jade_scene_set_textures) against the untextured render: what DESIGN.md 3.20 quotes.

usage: python tools/texture_ab.py [--out profiles/texture_ab.json] [--configs C2,C3] [--frames 16] [--spp 64] [--converged-spp 4096]
           C2 at 512 x 512 and C3 at 1920 x 1080.  The floor (object 2, a box: planar UVs from above) carries a 1024 x 1024 checker of
           64 x 64 squares, the statue (object 0) a 2048 x 2048 image through spherical_uvs.
             cost     --frames frames of --spp samples each after a warm-up frame, device time from jade_stats, three renders alternating
                      frame by frame: the textured render (it runs the list schedule), the untextured render under the same list schedule
                      (JADE_FUSED=0 JADE_TAIL=0, read when the handle is made) and the untextured render under the default schedule.
                      Both ratios are written down - the second includes the price of losing the fused first pass and is what a user
                      pays - and the time per ray of each, so that the lookup's share shows: a texture adds no ray.
             denoise  relMSE of the denoised --spp frame against a --converged-spp render of the same (textured) scene, mean over pixels
                      and channels of (x - ref)^2 / (ref^2 + 1e-4), over the whole frame and over the pixels whose centre ray lands on
                      the floor within two texels of a checker edge - with the textured render's own albedo guide (jade_render_denoise),
                      and with the untextured scene's albedo guide in its place (jade_denoise_image on the same frame, variance, normal
                      and depth).  Whether the textured guide keeps the checker's edges is the claim under test.
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
STATUE, FLOOR = 0, 2
CHECKER, SQUARES = 1024, 64


def statue_image(size=2048):
    """A veined stone in linear RGB, 0.25 .. 1: sums of sines of (u, v), periodic in both, so that the seam does not show."""
    v, u = np.meshgrid(np.arange(size) / size, np.arange(size) / size, indexing="ij")
    t = 2 * np.pi
    vein = np.sin(t * (3 * u + 2 * v) + 2.5 * np.sin(t * (2 * v - u)) + 1.5 * np.sin(t * 5 * u))
    fine = np.sin(t * 37 * u) * np.sin(t * 29 * v)
    g = 0.65 + 0.25 * vein + 0.1 * fine
    return np.stack([0.85 * g, g, 0.8 * g + 0.1], -1).astype(np.float32)


def build(name, textured):
    b = H.SceneBuilder()
    try:
        if textured:
            b.set_object_texture(STATUE, statue_image(), H.UV_SPHERICAL)
            b.set_object_texture(FLOOR, H.texture_checker(CHECKER, SQUARES, (0.9, 0.9, 0.9), (0.15, 0.15, 0.15)), H.UV_PLANAR_Y)
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


def edge_pixels(sc, hs, p):
    """The pixels whose centre ray lands on a checker-textured triangle within two texels of a checker edge: [H, W] bool."""
    images, uv, image_of = hs.textures
    w, h = p.width, p.height
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    lx = (-1 + 2.0 / w * x) * (w / h)                     # (the pixel's centre: both jitter draws at 0.5)
    ly = -1 + 2.0 / h * y
    M = np.asarray(list(p.camera), np.float64).reshape(4, 4)
    d = lx[..., None] * M[0, :3] + ly[..., None] * M[1, :3] - 1.5 * M[2, :3]
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    o = np.broadcast_to(np.asarray(list(p.eye), np.float64), d.shape)
    idx, _, pt, _ = sc.trace_rays(o.reshape(-1, 3), d.reshape(-1, 3), np.full(w * h, -1, np.int32))
    checker = int(np.flatnonzero([im.shape[0] == CHECKER for im in images])[0])
    on = (idx >= 0) & (image_of[np.maximum(idx, 0)] == checker)
    k = np.where(on, idx, 0)
    v = hs.vertices().astype(np.float64)[k]
    e1, e2, wv = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], pt.astype(np.float64) - v[:, 0]
    n = np.cross(e1, e2)
    nn = np.maximum((n * n).sum(-1), 1e-300)
    b2, b3 = (np.cross(wv, e2) * n).sum(-1) / nn, (np.cross(e1, wv) * n).sum(-1) / nn
    t = uv[k].astype(np.float64)
    tex = (t[:, 0] + b2[:, None] * (t[:, 1] - t[:, 0]) + b3[:, None] * (t[:, 2] - t[:, 0])) * CHECKER
    cell = CHECKER / SQUARES
    near = np.abs(tex - np.round(tex / cell) * cell).min(-1) < 2.0
    return (on & near).reshape(h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_ab.json"))
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--converged-spp", type=int, default=4096)
    a = ap.parse_args()
    hip = J.hip()
    res = {"what": __doc__.strip().splitlines()[0], "frames": a.frames, "spp": a.spp, "converged_spp": a.converged_spp,
           "checker": [CHECKER, SQUARES], "configs": {}}
    for name in a.configs.split(","):
        size = SIZES[name]
        hs, cfg = build(name, True)
        plain_hs, _ = build(name, False)
        assert np.array_equal(hs.a["triangles"], plain_hs.a["triangles"])
        out = {"width": size[0], "height": size[1], "triangles": int(hs.n_triangles), "textured_triangles": int((hs.textures[2] >= 0).sum())}
        with scene_under(hip, plain_hs, {}) as plain_default, scene_under(hip, plain_hs, LIST) as plain_list, scene_under(hip, hs, {}) as textured:
            runs = {"textured": (textured, []), "plain_list": (plain_list, []), "plain_default": (plain_default, [])}
            for frame in range(a.frames + 1):            # frame 0 warms up
                for key, (sc, ms) in runs.items():
                    st = sc.render(params(cfg, size, a.spp, 1000 * frame), want_rgb=False, want_bgr8=False)[2]
                    if frame:
                        ms.append(dict(kernel_ms=st.kernel_ms, rays=st.rays, rays_inline=st.rays_inline, tail_launches=st.tail_launches))
            cost = {}
            for k, (_, ms) in runs.items():
                total, rays = float(sum(m["kernel_ms"] for m in ms)), int(sum(m["rays"] for m in ms))
                cost[k] = dict(frames=ms, kernel_ms_total=total, rays_total=rays, ns_per_ray=1e6 * total / rays)
            cost["textured_over_plain_list"] = cost["textured"]["kernel_ms_total"] / cost["plain_list"]["kernel_ms_total"]
            cost["textured_over_plain_default"] = cost["textured"]["kernel_ms_total"] / cost["plain_default"]["kernel_ms_total"]
            cost["same_rays"] = cost["textured"]["rays_total"] == cost["plain_list"]["rays_total"] == cost["plain_default"]["rays_total"]
            out["cost"] = cost
            ref = textured.render(params(cfg, size, a.converged_spp, 900000), want_bgr8=False)[0]
            p = params(cfg, size, a.spp, 5000)
            plain_default.render(p, want_rgb=False, want_bgr8=False)
            plain_albedo = plain_default.guides()["albedo"]
            raw = textured.render(p, want_bgr8=False)[0]
            g = textured.guides()
            den_own = textured.denoise(want_bgr8=False)[0]
            den_same = hip.denoise_image(raw, g["variance"], g["albedo"], g["normal"], g["depth"])       # the same filter through the image entry
            den_plain = hip.denoise_image(raw, g["variance"], plain_albedo, g["normal"], g["depth"])
            keep = edge_pixels(textured, hs, p)
            out["denoise"] = dict(edge_pixels=int(keep.sum()),
                                  image_entry_equals_render_entry=bool(np.array_equal(den_own.view(np.uint32), den_same.view(np.uint32))),
                                  rel_mse_raw=rel_mse(raw, ref), rel_mse_raw_edge_pixels=rel_mse(raw, ref, keep),
                                  rel_mse_textured_guide=rel_mse(den_own, ref), rel_mse_textured_guide_edge_pixels=rel_mse(den_own, ref, keep),
                                  rel_mse_plain_guide=rel_mse(den_plain, ref), rel_mse_plain_guide_edge_pixels=rel_mse(den_plain, ref, keep))
        res["configs"][name] = out
        c, d = out["cost"], out["denoise"]
        print(f"{name}: textured / plain (list schedule) {c['textured_over_plain_list']:.3f}, textured / plain (default schedule) {c['textured_over_plain_default']:.3f}; "
              f"ns per ray {c['textured']['ns_per_ray']:.4f} / {c['plain_list']['ns_per_ray']:.4f} / {c['plain_default']['ns_per_ray']:.4f}; same rays {c['same_rays']}; "
              f"denoised relMSE whole frame: textured guide {d['rel_mse_textured_guide']:.4g}, plain guide {d['rel_mse_plain_guide']:.4g}, raw {d['rel_mse_raw']:.4g}; "
              f"on {d['edge_pixels']} edge pixels: {d['rel_mse_textured_guide_edge_pixels']:.4g}, {d['rel_mse_plain_guide_edge_pixels']:.4g}, "
              f"{d['rel_mse_raw_edge_pixels']:.4g}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
