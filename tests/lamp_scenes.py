"""The lamp scenes of the sampling modes (one-light, cosine bounces, MIS): a slab, a ball and a small jade box under a geodesic lamp and
two quad lights, with emitter lists of 84, 82, 3, 1, 0 and 81 924 entries.  Built on the host, once per process."""
import numpy as np

from jaderaytracerendering_amd import _abi, backend as B, host as H
from jaderaytracerendering_amd.host import HostScene

W, HH, SPP = 48, 40, 6
QUAD_I = np.int32([[0, 1, 2], [0, 2, 3]])


def _jade():
    return H.material(brdf=(0.3, 0.4, 0.5), reflex_mode=_abi.MIRROR, refract_mode=_abi.SUB_SURFACE, refract_rate=(0.3, 0.4, 0.5),
                      refract_albedo=(0.3, 0.5, 0.7), refract_index=2.66)


def _build(freq):
    """A diffuse slab, a diffuse ball, a small SUB_SURFACE box (so the diffuse, the SSS-diffuse and the BSSRDF branch all sample the
    emitters), a geodesic lamp of 20 freq^2 triangles and two quad lights of unequal power, under a 16 x 8 sky."""
    b = H.SceneBuilder()
    try:
        T = H.transform_matrix
        b.add_proc("box", 0, H.material(brdf=(0.6, 0.5, 0.4)), T(trans=(0, -1.1, 0), scale=(7, 0.2, 7)))
        b.add_proc("geodesic", 2, H.material(brdf=(0.5, 0.6, 0.5)), T(trans=(-1.1, -0.45, 0.2), scale=(0.5,) * 3))
        b.add_proc("box", 0, _jade(), T(rot_deg=(0, 35, 0), trans=(0.55, -0.7, 0.9), scale=(0.6,) * 3))
        b.add_proc("geodesic", freq, H.material(emissive=(30, 27, 22), brdf=(0.3,) * 3), T(trans=(0.3, 1.3, 0.4), scale=(0.25,) * 3))
        big = np.float32([[-2.6, 0.2, -1.8], [-1.4, 0.2, -1.8], [-1.4, 1.4, -1.8], [-2.6, 1.4, -1.8]])
        b.add_mesh(big, QUAD_I, H.material(emissive=(9, 12, 15), brdf=(0.3,) * 3))
        small = np.float32([[1.8, -0.6, 1.6], [2.1, -0.6, 1.3], [2.1, -0.3, 1.3], [1.8, -0.3, 1.6]])
        b.add_mesh(small, QUAD_I, H.material(emissive=(40, 10, 4), brdf=(0.3,) * 3))
        b.set_env_sky(16, 8)
        return b.build()
    finally:
        b.close()


_scenes = {}


def lamp_scene(name="lamp"):
    """"lamp": the 80-triangle lamp and the two quads, 84 entries.  "lamp82" / "lamp3" / "lamp1": the same triangles with 82 (the lamp
    and one triangle of each quad), 3 and 1 of them listed - an emissive triangle need not be listed (it is then found by hitting it
    only).  "none": none listed.  "big": the lamp at frequency 64, 81 920 + 4 entries."""
    if name not in _scenes:
        if name == "lamp":
            hs = _build(2)
            assert len(hs.a["emit"]) == 84
        elif name == "big":
            hs = _build(64)
            assert len(hs.a["emit"]) == 81924
        else:
            base = lamp_scene("lamp")
            hs = HostScene({k: np.array(v, copy=True) for k, v in base.a.items()}, base.bvh_depth)
            e = base.a["emit"]
            tf = base.tri_f32()
            lamp = [i for i in e if tf[i, 13] == 30]
            quads = [i for i in e if tf[i, 13] != 30]
            assert len(lamp) == 80 and len(quads) == 4
            pick = {"lamp82": lamp + [quads[0], quads[2]], "lamp3": [lamp[7], quads[0], quads[3]], "lamp1": [quads[1]], "none": []}[name]
            hs.a["emit"] = np.int32(pick)
        _scenes[name] = hs
    return _scenes[name]


def params(spp=SPP, w=W, h=HH, **kw):
    eye, cam = H.camera_orbit(5.0, 20.0, 30.0)
    return B.make_params(w, h, spp, eye, cam, **kw)
