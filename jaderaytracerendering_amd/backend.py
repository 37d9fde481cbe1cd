"""Binding of the jade_rt.h C ABI.

`hip()` returns the product backend (libjade_hip.so, hand-written HIP for
gfx950) and raises if it is missing — there is no CPU fallback in the product
path.  `Backend(path)` binds any library implementing jade_rt.h; the test
suite uses it to load the CPU oracle as the checker.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

_LIBDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
HIP_LIB = os.path.join(_LIBDIR, "libjade_hip.so")


class JadeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"jade_rt status {code}: {msg}")
        self.code = code


def make_params(width, height, spp, eye, camera, frame=0, tile_rank=0, tile_nranks=1, device_id=0, threads=0, walk=_abi.WALK_REFERENCE, env_sampling=_abi.ENV_REFERENCE):
    p = _abi.RenderParams()
    p.width, p.height, p.spp, p.frame = int(width), int(height), int(spp), int(frame)
    p.eye[:] = [float(v) for v in eye]
    p.camera[:] = [float(v) for v in camera]
    p.tile_rank, p.tile_nranks = int(tile_rank), int(tile_nranks)
    p.device_id, p.threads = int(device_id), int(threads)
    p.walk = int(walk)  # jade_rt.h, JADE_WALK_*: 0 = the reference's walk (V / T equal the oracle's), 1 = early exits, 2 = + occluder cache
    p.env_sampling = int(env_sampling)  # JADE_ENV_*: 0 = the reference's estimator; 1 = environment rays by importance, 2 = importance mixed with the hemisphere draw (non-parity)
    return p


def params_from_config(cfg, **kw):
    kw.setdefault("spp", cfg.spp)
    return make_params(cfg.width, cfg.height, kw.pop("spp"), list(cfg.eye), list(cfg.camera), **kw)


class Meter:
    """jade_meter (include/jade_bvh.h): the luminance histogram of a frame - `bins` (uint64 [512], 8 per stop over [2^-32, 2^32)), the
    counts of the zero, negative and non-finite pixels, and the smallest and largest positive luminance (float32; 0 without positive
    pixels).  Integers, so meters add: `a + b` is the meter of two ranks' tiles together."""

    def __init__(self, bins=None, n_zero=0, n_negative=0, n_nonfinite=0, lum_min=0.0, lum_max=0.0):
        self.bins = np.zeros(_abi.METER_BINS, np.uint64) if bins is None else np.array(bins, np.uint64).reshape(_abi.METER_BINS)
        self.n_zero, self.n_negative, self.n_nonfinite = int(n_zero), int(n_negative), int(n_nonfinite)
        self.lum_min, self.lum_max = np.float32(lum_min), np.float32(lum_max)

    @property
    def n_positive(self):
        return int(self.bins.sum())

    @property
    def total(self):
        """Pixels metered: the four classes together."""
        return self.n_positive + self.n_zero + self.n_negative + self.n_nonfinite

    @classmethod
    def from_struct(cls, m):
        return cls(np.ctypeslib.as_array(m.bins).copy(), m.n_zero, m.n_negative, m.n_nonfinite, m.lum_min, m.lum_max)

    def to_struct(self):
        m = _abi.MeterStruct()
        m.bins[:] = [int(v) for v in self.bins]
        m.n_positive, m.n_zero, m.n_negative, m.n_nonfinite = self.n_positive, self.n_zero, self.n_negative, self.n_nonfinite
        m.lum_min, m.lum_max = float(self.lum_min), float(self.lum_max)
        return m

    def __add__(self, other):
        both = [m for m in (self, other) if m.n_positive]
        return Meter(self.bins + other.bins, self.n_zero + other.n_zero, self.n_negative + other.n_negative,
                     self.n_nonfinite + other.n_nonfinite, min((m.lum_min for m in both), default=0.0),
                     max((m.lum_max for m in both), default=0.0))

    def __eq__(self, other):
        return (isinstance(other, Meter) and np.array_equal(self.bins, other.bins)
                and (self.n_zero, self.n_negative, self.n_nonfinite) == (other.n_zero, other.n_negative, other.n_nonfinite)
                and self.lum_min.tobytes() == other.lum_min.tobytes() and self.lum_max.tobytes() == other.lum_max.tobytes())

    __hash__ = None

    def __repr__(self):
        return (f"Meter(positive={self.n_positive}, zero={self.n_zero}, negative={self.n_negative}, nonfinite={self.n_nonfinite}, "
                f"lum=[{self.lum_min!r}, {self.lum_max!r}])")

    @staticmethod
    def bin_edges():
        """float64 [513]: bin b covers [edges[b], edges[b + 1]) - 2^E (1 + k/8) with E = (b >> 3) - 32, k = b & 7."""
        b = np.arange(_abi.METER_BINS + 1)
        return np.ldexp(1.0 + (b & 7) / 8.0, (b >> 3) - 32)


class Backend:
    def __init__(self, path):
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it first (make / __graft_entry__.build())")
        self.path = path
        self.lib = _abi.bind(C.CDLL(path), _abi.RT_SYMBOLS)
        if self.lib.jade_abi_version() != _abi.JADE_ABI_VERSION:
            raise RuntimeError(f"{path}: ABI version mismatch")

    @property
    def name(self):
        return self.lib.jade_backend_name().decode()

    def check(self, rc):
        if rc != 0:
            raise JadeError(rc, self.lib.jade_last_error().decode())

    def device_count(self):
        n = C.c_int(0)
        self.check(self.lib.jade_device_count(C.byref(n)))
        return n.value

    def scene(self, host_scene, device_id=0):
        return Scene(self, host_scene, device_id)

    def owned_tile_count(self, width, height, rank, nranks):
        return self.lib.jade_owned_tile_count(width, height, rank, nranks)

    def hip_only(self, name):
        """An include/jade_bvh.h entry point: JadeError(JADE_ERR_UNSUPPORTED) on a backend without it (the oracle)."""
        fn = getattr(self.lib, name, None)
        if fn is None:
            raise JadeError(_abi.JADE_ERR_UNSUPPORTED, f"{self.path} has no {name} (HIP module only)")
        fn.restype, fn.argtypes = _abi.BVH_SYMBOLS[name]
        return fn

    def denoise_defaults(self):
        """jade_denoise_defaults: the DenoiseParams DESIGN.md 3.6 chose."""
        p = _abi.DenoiseParams()
        self.hip_only("jade_denoise_defaults")(C.byref(p))
        return p

    def denoise_image(self, rgb, variance, albedo, normal, depth, params=None, device_id=0):
        """jade_denoise_image: the edge-aware filter (include/jade_bvh.h) on caller images - rgb, albedo, normal [H, W, 3], variance,
        depth [H, W] - on device `device_id`.  params None: the defaults.  Returns the filtered rgb, float32 [H, W, 3]."""
        fn = self.hip_only("jade_denoise_image")
        if params is None:
            params = self.denoise_defaults()
        rgb = np.ascontiguousarray(rgb, np.float32)
        h, w = rgb.shape[:2]
        ins = [np.ascontiguousarray(a, np.float32) for a in (variance, albedo, normal, depth)]
        for a, shape in zip(ins, ((h, w), (h, w, 3), (h, w, 3), (h, w))):
            if a.shape != shape:
                raise ValueError(f"input of shape {a.shape}, expected {shape}")
        out = np.zeros((h, w, 3), np.float32)
        self.check(fn(int(device_id), int(w), int(h), rgb.ctypes.data, *[a.ctypes.data for a in ins], C.byref(params), out.ctypes.data))
        return out


    def display_defaults(self):
        """jade_display_defaults: ACES, manual exposure 1; key 0.18, window [0.05, 0.95], clamp [2^-16, 2^16] for auto."""
        p = _abi.DisplayParams()
        self.hip_only("jade_display_defaults")(C.byref(p))
        return p

    def display_params(self, exposure, tonemap=None, limit=1.5):
        """The DisplayParams of an `exposure` argument: a DisplayParams is taken as it is; a number is a manual multiplier; "auto"
        is the defaults' histogram policy.  tonemap None: ACES."""
        if isinstance(exposure, _abi.DisplayParams):
            return exposure
        p = self.display_defaults()
        p.tonemap, p.limit = _abi.TONEMAP_ACES if tonemap is None else int(tonemap), float(limit)
        if isinstance(exposure, str):
            if exposure != "auto":
                raise ValueError(f"exposure {exposure!r}: a number, \"auto\" or a DisplayParams")
            p.exposure_mode = _abi.EXPOSURE_AUTO
        else:
            p.exposure_mode, p.exposure = _abi.EXPOSURE_MANUAL, float(exposure)
        return p

    def meter_exposure(self, meter, display):
        """jade_meter_exposure: the exposure `display` chooses for `meter` (a Meter; may be None under manual), a float holding
        the float32 value.  Host code: needs no GPU.  JadeError(JADE_ERR_INVALID) for parameters outside their ranges."""
        fn = self.hip_only("jade_meter_exposure")
        e = fn(C.byref(meter.to_struct()) if meter is not None else None, C.byref(display))
        if e != e:
            raise JadeError(_abi.JADE_ERR_INVALID, self.lib.jade_last_error().decode())
        return e

    def expose_image(self, rgb, display=None, want_bgr8=True, device_id=0):
        """jade_expose_image: meter, exposure and tone pack of a caller's frame rgb [H, W, 3] (a denoised frame, the gathered frame of
        several ranks) on device `device_id`.  display None: the defaults.  Returns (bgr8 uint8 [H, W, 3] | None, exposure, Meter)."""
        fn = self.hip_only("jade_expose_image")
        if display is None:
            display = self.display_defaults()
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"rgb of shape {rgb.shape}, expected [H, W, 3]")
        h, w = rgb.shape[:2]
        bgr = np.zeros((h, w, 3), np.uint8) if want_bgr8 else None
        e, m = C.c_float(0.0), _abi.MeterStruct()
        self.check(fn(int(device_id), int(w), int(h), rgb.ctypes.data, C.byref(display), bgr.ctypes.data if want_bgr8 else None,
                      C.byref(e), C.byref(m)))
        return bgr, e.value, Meter.from_struct(m)

    def glare_defaults(self):
        """jade_glare_defaults: 6 levels, strength 0.1, falloff 0.5 - a look, not a measurement."""
        p = _abi.GlareParams()
        self.hip_only("jade_glare_defaults")(C.byref(p))
        return p

    def glare_image(self, rgb, params=None, device_id=0):
        """jade_glare_image: the bloom pyramid (include/jade_bvh.h) on a caller's linear frame rgb [H, W, 3] (a denoised frame, the
        gathered frame of several ranks) on device `device_id`.  params None: the defaults.  Returns the glared rgb, float32 [H, W, 3]."""
        fn = self.hip_only("jade_glare_image")
        if params is None:
            params = self.glare_defaults()
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"rgb of shape {rgb.shape}, expected [H, W, 3]")
        h, w = rgb.shape[:2]
        out = np.zeros((h, w, 3), np.float32)
        self.check(fn(int(device_id), int(w), int(h), rgb.ctypes.data, C.byref(params), out.ctypes.data))
        return out

    def despeckle_defaults(self):
        """jade_despeckle_defaults: 1 iteration, radius 1, rank 2, gain 2, floor 0, sigmas 2."""
        p = _abi.DespeckleParams()
        self.hip_only("jade_despeckle_defaults")(C.byref(p))
        return p

    def despeckle_image(self, rgb, variance=None, params=None, device_id=0):
        """jade_despeckle_image: the despeckle passes (include/jade_bvh.h, "Despeckle, stated") on a caller's linear frame rgb [H, W, 3]
        and, optionally, the variance [H, W] of each pixel's mean luminance (Scene.guides) on device `device_id`.  params None: the
        defaults.  Returns (rgb float32 [H, W, 3], variance float32 [H, W] | None, scale float32 [H, W], the report as a dict of its
        four counts)."""
        fn = self.hip_only("jade_despeckle_image")
        if params is None:
            params = self.despeckle_defaults()
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"rgb of shape {rgb.shape}, expected [H, W, 3]")
        h, w = rgb.shape[:2]
        if variance is not None:
            variance = np.ascontiguousarray(variance, np.float32)
            if variance.shape != (h, w):
                raise ValueError(f"variance of shape {variance.shape}, expected {(h, w)}")
        out = np.zeros((h, w, 3), np.float32)
        out_v = np.zeros((h, w), np.float32) if variance is not None else None
        scale = np.zeros((h, w), np.float32)
        rep = _abi.DespeckleReport()
        self.check(fn(int(device_id), int(w), int(h), rgb.ctypes.data, variance.ctypes.data if variance is not None else None,
                      C.byref(params), out.ctypes.data, out_v.ctypes.data if out_v is not None else None, scale.ctypes.data, C.byref(rep)))
        return out, out_v, scale, despeckle_report(rep)


def despeckle_report(rep):
    """jade_despeckle_report as a dict; reports add field by field"""
    return {k: int(getattr(rep, k)) for k in ("n_usable", "n_above", "n_established", "n_clamped")}


class Scene:
    """A scene resident on the backend (PathTrace.cu:1618-1698 on the reference side)."""

    def __init__(self, backend, host_scene, device_id=0):
        self.backend = backend
        self.host_scene = host_scene
        self._h = C.c_void_p()
        desc = host_scene.desc()
        backend.check(backend.lib.jade_scene_create(C.byref(desc), device_id, C.byref(self._h)))
        self._params = None
        if getattr(host_scene, "vertex_normals", None) is not None:  # a host scene without a table behaves as it always did
            try:
                self.set_vertex_normals(host_scene.vertex_normals)
            except Exception:
                self.close()
                raise
        if getattr(host_scene, "textures", None) is not None:  # ... and the same for its textures: (images, uv, image_of)
            try:
                self.set_textures(*host_scene.textures)
            except Exception:
                self.close()
                raise
        if getattr(host_scene, "normal_maps", None) is not None:  # ... and its normal maps: (images, uv, image_of, strength)
            try:
                self.set_normal_maps(*host_scene.normal_maps)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.backend.lib.jade_scene_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def render(self, params, want_rgb=True, want_bgr8=True):
        """(rgb float32 [H,W,3] | None, bgr8 uint8 [H,W,3] | None, Stats); row 0 = bottom row."""
        h, w = params.height, params.width
        rgb = np.zeros((h, w, 3), np.float32) if want_rgb else None
        bgr = np.zeros((h, w, 3), np.uint8) if want_bgr8 else None
        st = _abi.Stats()
        self.backend.check(self.backend.lib.jade_render(self._h, C.byref(params), rgb.ctypes.data if want_rgb else None,
                                                        bgr.ctypes.data if want_bgr8 else None, C.byref(st)))
        self._params = params  # (jade_render is begin + step + resolve: the render stays readable, e.g. by error_map)
        return rgb, bgr, st

    # progressive form
    def begin(self, params):
        self._params = params
        self.backend.check(self.backend.lib.jade_render_begin(self._h, C.byref(params)))

    def step(self, spp, stats=None):
        st = stats if stats is not None else _abi.Stats()
        self.backend.check(self.backend.lib.jade_render_step(self._h, int(spp), C.byref(st)))
        return st

    def flush(self, stats=None):
        """Finish the paths a step may have carried over (jade_rt.h); resolve() does it implicitly."""
        st = stats if stats is not None else _abi.Stats()
        self.backend.check(self.backend.lib.jade_render_flush(self._h, C.byref(st)))
        return st

    def resolve(self, want_rgb=True, want_bgr8=True, tonemap=None, limit=1.5, exposure=None):
        """tonemap None/ACES: PathTrace.cu:680-682; _abi.TONEMAP_REINHARD: the preview's pass3.fsh operator.
        exposure None: (rgb, bgr8) of jade_render_resolve / _resolve_ex.  Otherwise jade_render_resolve_exposed (HIP module only): a
        number is a manual multiplier, "auto" the histogram policy with the defaults, a DisplayParams is taken as it is (tonemap and
        limit included); returns (rgb - never scaled, bgr8 of exposure x rgb, the exposure used, the Meter of this rank's pixels)."""
        h, w = self._params.height, self._params.width
        rgb = np.zeros((h, w, 3), np.float32) if want_rgb else None
        bgr = np.zeros((h, w, 3), np.uint8) if want_bgr8 else None
        pr, pb = (rgb.ctypes.data if want_rgb else None), (bgr.ctypes.data if want_bgr8 else None)
        if exposure is not None:
            fn = self._hip_only("jade_render_resolve_exposed")
            dp = self.backend.display_params(exposure, tonemap, limit)
            e, m = C.c_float(0.0), _abi.MeterStruct()
            self.backend.check(fn(self._h, C.byref(dp), pr, pb, C.byref(e), C.byref(m)))
            return rgb, bgr, e.value, Meter.from_struct(m)
        if tonemap is None:
            self.backend.check(self.backend.lib.jade_render_resolve(self._h, pr, pb))
        else:
            self.backend.check(self.backend.lib.jade_render_resolve_ex(self._h, int(tonemap), float(limit), pr, pb))
        return rgb, bgr

    def _hip_only(self, name):
        """An include/jade_bvh.h entry point: JadeError(JADE_ERR_UNSUPPORTED) on a backend without it (the oracle)."""
        fn = getattr(self.backend.lib, name, None)
        if fn is None:
            raise JadeError(_abi.JADE_ERR_UNSUPPORTED, f"{self.backend.path} has no {name} (HIP module only)")
        fn.restype, fn.argtypes = _abi.BVH_SYMBOLS[name]
        return fn

    def render_adaptive(self, params, min_spp, rel_error, error_floor=0.01, want_rgb=True, want_bgr8=True):
        """jade_render_adaptive: params.spp is the cap; each 16x16 tile stops at the first of min_spp, 2 min_spp, ... whose tile
        error is <= rel_error.  Returns (rgb | None, bgr8 | None, tile_spp int32 [tiles_y, tiles_x] (0 = not owned), Stats)."""
        fn = self._hip_only("jade_render_adaptive")
        h, w = params.height, params.width
        ts = _abi.TILE_SIZE
        rgb = np.zeros((h, w, 3), np.float32) if want_rgb else None
        bgr = np.zeros((h, w, 3), np.uint8) if want_bgr8 else None
        tile_spp = np.zeros(((h + ts - 1) // ts, (w + ts - 1) // ts), np.int32)
        st = _abi.Stats()
        self.backend.check(fn(self._h, C.byref(params), int(min_spp), float(rel_error), float(error_floor),
                              rgb.ctypes.data if want_rgb else None, bgr.ctypes.data if want_bgr8 else None,
                              tile_spp.ctypes.data, C.byref(st)))
        self._params = params
        return rgb, bgr, tile_spp, st

    def error_map(self, error_floor=0.01):
        """jade_render_error: [H, W] float32 relative standard error of each pixel's mean luminance (include/jade_bvh.h) for the
        render in progress; NaN on tiles this rank does not own and where the sample count cannot be estimated."""
        fn = self._hip_only("jade_render_error")
        if self._params is None:
            raise JadeError(_abi.JADE_ERR_INVALID, "jade_render_begin not called")
        out = np.full((self._params.height, self._params.width), np.nan, np.float32)
        self.backend.check(fn(self._h, float(error_floor), out.ctypes.data))
        return out

    def guides(self, guide_spp=4):
        """jade_render_guides: the denoiser's inputs for the render in progress, a dict of float32 arrays - "albedo", "normal"
        [H, W, 3], "depth", "variance" [H, W] - laid out as resolve's; tiles this rank does not own are NaN."""
        fn = self._hip_only("jade_render_guides")
        if self._params is None:
            raise JadeError(_abi.JADE_ERR_INVALID, "jade_render_begin not called")
        h, w = self._params.height, self._params.width
        out = {"albedo": np.full((h, w, 3), np.nan, np.float32), "normal": np.full((h, w, 3), np.nan, np.float32),
               "depth": np.full((h, w), np.nan, np.float32), "variance": np.full((h, w), np.nan, np.float32)}
        self.backend.check(fn(self._h, int(guide_spp), out["albedo"].ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data,
                              out["variance"].ctypes.data))
        return out

    def denoise(self, params=None, tonemap=None, limit=1.5, want_rgb=True, want_bgr8=True):
        """jade_render_denoise: the render in progress, filtered on its device (full frame only).  params None: the defaults;
        tonemap None: ACES.  Returns (rgb float32 [H, W, 3] | None, bgr8 uint8 [H, W, 3] | None)."""
        fn = self._hip_only("jade_render_denoise")
        if self._params is None:
            raise JadeError(_abi.JADE_ERR_INVALID, "jade_render_begin not called")
        if params is None:
            params = self.backend.denoise_defaults()
        h, w = self._params.height, self._params.width
        rgb = np.zeros((h, w, 3), np.float32) if want_rgb else None
        bgr = np.zeros((h, w, 3), np.uint8) if want_bgr8 else None
        self.backend.check(fn(self._h, C.byref(params), _abi.TONEMAP_ACES if tonemap is None else int(tonemap), float(limit),
                              rgb.ctypes.data if want_rgb else None, bgr.ctypes.data if want_bgr8 else None))
        return rgb, bgr

    def glare(self, params=None, display=None, want_rgb=True, want_bgr8=True):
        """jade_render_glare: the render in progress, glared on its device (full frame only), metered and tone-packed.  params None:
        the glare defaults; display None: jade_display_defaults.  Returns (rgb float32 [H, W, 3] | None - the glared linear frame,
        never scaled, bgr8 uint8 [H, W, 3] | None, the exposure used)."""
        fn = self._hip_only("jade_render_glare")
        if self._params is None:
            raise JadeError(_abi.JADE_ERR_INVALID, "jade_render_begin not called")
        if params is None:
            params = self.backend.glare_defaults()
        h, w = self._params.height, self._params.width
        rgb = np.zeros((h, w, 3), np.float32) if want_rgb else None
        bgr = np.zeros((h, w, 3), np.uint8) if want_bgr8 else None
        e = C.c_float(0.0)
        self.backend.check(fn(self._h, C.byref(params), C.byref(display) if display is not None else None,
                              rgb.ctypes.data if want_rgb else None, bgr.ctypes.data if want_bgr8 else None, C.byref(e)))
        return rgb, bgr, e.value

    def despeckle(self, params=None, denoise=None, tonemap=None, limit=1.5, want_rgb=True, want_bgr8=True):
        """jade_render_despeckle: the render in progress, despeckled on its device (full frame only) and tone-packed.  params None: the
        despeckle defaults.  denoise: DenoiseParams to run the guides and the a-trous filter on the despeckled colour and variance,
        None for the despeckled frame itself.  Returns (rgb float32 [H, W, 3] | None, bgr8 uint8 [H, W, 3] | None, scale float32
        [H, W], the report as a dict of its four counts)."""
        fn = self._hip_only("jade_render_despeckle")
        if self._params is None:
            raise JadeError(_abi.JADE_ERR_INVALID, "jade_render_begin not called")
        if params is None:
            params = self.backend.despeckle_defaults()
        h, w = self._params.height, self._params.width
        rgb = np.zeros((h, w, 3), np.float32) if want_rgb else None
        bgr = np.zeros((h, w, 3), np.uint8) if want_bgr8 else None
        scale = np.zeros((h, w), np.float32)
        rep = _abi.DespeckleReport()
        self.backend.check(fn(self._h, C.byref(params), C.byref(denoise) if denoise is not None else None,
                              _abi.TONEMAP_ACES if tonemap is None else int(tonemap), float(limit),
                              rgb.ctypes.data if want_rgb else None, bgr.ctypes.data if want_bgr8 else None, scale.ctypes.data, C.byref(rep)))
        return rgb, bgr, scale, despeckle_report(rep)

    def set_lens(self, aperture_radius, focus_distance=0.0):
        """jade_scene_set_lens: a thin lens of radius `aperture_radius` (scene units) focused at depth `focus_distance` along the
        camera's axis, for every render this handle begins from now on (HIP module only; non-parity: include/jade_bvh.h, "The lens,
        stated").  set_lens(None), or a radius of 0: the pinhole.  JadeError(JADE_ERR_INVALID) leaves the previous lens in place."""
        fn = self._hip_only("jade_scene_set_lens")
        if aperture_radius is None:
            self.backend.check(fn(self._h, None))
            return
        lens = _abi.LensParams(float(aperture_radius), float(focus_distance))
        self.backend.check(fn(self._h, C.byref(lens)))

    def lens(self):
        """jade_scene_get_lens: (aperture_radius, focus_distance) as set; (0.0, 0.0) for a handle that never got a lens."""
        fn = self._hip_only("jade_scene_get_lens")
        lens = _abi.LensParams()
        self.backend.check(fn(self._h, C.byref(lens)))
        return lens.aperture_radius, lens.focus_distance

    def set_shutter(self, eye_close, camera_close=None, t_open=0.0, t_close=1.0):
        """jade_scene_set_shutter: every render this handle begins from now on opens its shutter at the pose of its params and closes it at
        (eye_close, camera_close); each sample is traced from the pose at a time of its own within [t_open, t_close] of that move (HIP
        module only; non-parity: include/jade_bvh.h, "The shutter, stated").  set_shutter(None) removes it.
        JadeError(JADE_ERR_INVALID) leaves the previous shutter in place."""
        fn = self._hip_only("jade_scene_set_shutter")
        if eye_close is None:
            self.backend.check(fn(self._h, None))
            return
        e = np.asarray(eye_close, np.float32).ravel()
        m = np.asarray(camera_close, np.float32).ravel()
        if e.shape != (3,) or m.shape != (16,):
            raise ValueError("set_shutter wants eye_close[3] and camera_close[16]")
        sh = _abi.ShutterParams(_abi.f3(*e.tolist()), (C.c_float * 16)(*m.tolist()), float(t_open), float(t_close))
        self.backend.check(fn(self._h, C.byref(sh)))

    def shutter(self):
        """jade_scene_get_shutter: (eye_close[3], camera_close[16], t_open, t_close) as set, or None for a handle without a shutter."""
        fn = self._hip_only("jade_scene_get_shutter")
        sh = _abi.ShutterParams()
        is_set = C.c_int(0)
        self.backend.check(fn(self._h, C.byref(sh), C.byref(is_set)))
        if not is_set.value:
            return None
        return np.array(sh.eye_close[:], np.float32), np.array(sh.camera_close[:], np.float32), sh.t_open, sh.t_close

    def set_light_sampling(self, mode):
        """jade_scene_set_light_sampling: _abi.LIGHTS_ALL (the default: a shadow ray to every emitter entry at every sampling vertex, as the
        reference does) or _abi.LIGHTS_ONE (one entry per vertex, drawn by power and weighted by 1 / its probability; HIP module only;
        non-parity: include/jade_bvh.h, "The lights, stated").  Taken by the next render this handle begins.
        JadeError(JADE_ERR_INVALID) leaves the previous mode in place."""
        fn = self._hip_only("jade_scene_set_light_sampling")
        self.backend.check(fn(self._h, int(mode)))

    @property
    def light_sampling(self):
        """jade_scene_get_light_sampling: the mode the next render of this handle takes."""
        fn = self._hip_only("jade_scene_get_light_sampling")
        mode = C.c_int(-1)
        self.backend.check(fn(self._h, C.byref(mode)))
        return mode.value

    def set_bounce_sampling(self, mode):
        """jade_scene_set_bounce_sampling: _abi.BOUNCE_UNIFORM (the default: environment and indirect rays uniform over the hemisphere, as
        the reference draws them) or _abi.BOUNCE_COSINE (drawn with pdf cos / pi about the normal, the cosine taken out of the weight; HIP
        module only; non-parity: include/jade_bvh.h, "The bounce, stated").  Taken by the next render this handle begins.
        JadeError(JADE_ERR_INVALID) leaves the previous mode in place."""
        fn = self._hip_only("jade_scene_set_bounce_sampling")
        self.backend.check(fn(self._h, int(mode)))

    @property
    def bounce_sampling(self):
        """jade_scene_get_bounce_sampling: the mode the next render of this handle takes."""
        fn = self._hip_only("jade_scene_get_bounce_sampling")
        mode = C.c_int(-1)
        self.backend.check(fn(self._h, C.byref(mode)))
        return mode.value

    def set_direct_sampling(self, mode):
        """jade_scene_set_direct_sampling: _abi.DIRECT_RAYS (the default: the emitter rays alone gather the listed emitters' light) or
        _abi.DIRECT_MIS (the emitter rays and the indirect ray weighed against each other with the balance heuristic; needs
        _abi.BOUNCE_COSINE at the next render; HIP module only; non-parity: include/jade_bvh.h, "The direct light, stated").  Taken by the
        next render this handle begins.  JadeError(JADE_ERR_INVALID) leaves the previous mode in place."""
        fn = self._hip_only("jade_scene_set_direct_sampling")
        self.backend.check(fn(self._h, int(mode)))

    @property
    def direct_sampling(self):
        """jade_scene_get_direct_sampling: the mode the next render of this handle takes."""
        fn = self._hip_only("jade_scene_get_direct_sampling")
        mode = C.c_int(-1)
        self.backend.check(fn(self._h, C.byref(mode)))
        return mode.value

    def set_branch_sampling(self, mode):
        """jade_scene_set_branch_sampling: _abi.BRANCH_RANDOM (the default: every vertex tosses its coins - mirror or refraction arm, SSS or
        BSSRDF, the mirror's roulette - from the sample's stream, as the reference does) or _abi.BRANCH_STRATIFIED (at a path's first two
        vertices a pixel's samples share the arms out; HIP module only; non-parity: include/jade_bvh.h, "The branch draws, stated").  Taken by
        the next render this handle begins.  JadeError(JADE_ERR_INVALID) leaves the previous mode in place."""
        fn = self._hip_only("jade_scene_set_branch_sampling")
        self.backend.check(fn(self._h, int(mode)))

    @property
    def branch_sampling(self):
        """jade_scene_get_branch_sampling: the mode the next render of this handle takes."""
        fn = self._hip_only("jade_scene_get_branch_sampling")
        mode = C.c_int(-1)
        self.backend.check(fn(self._h, C.byref(mode)))
        return mode.value

    def set_vertex_normals(self, normals):
        """jade_scene_set_vertex_normals: float32 [n_triangles, 3, 3] (or anything of 9 n_triangles floats) - a normal per corner, corners in
        the order p1 p2 p3, triangles in the scene's order - or None to clear.  The next render this handle begins interpolates them at
        every path vertex (HIP module only; include/jade_bvh.h, "The shading normal, stated"); a table that is flat everywhere is today's
        render bit for bit."""
        fn = self._hip_only("jade_scene_set_vertex_normals")
        if normals is None:
            self.backend.check(fn(self._h, None, 0))
            return
        a = np.ascontiguousarray(normals, np.float32)
        if a.size % 9:
            raise JadeError(_abi.JADE_ERR_INVALID, "vertex normals: 9 floats per triangle")
        self.backend.check(fn(self._h, a.ctypes.data, a.size // 9))

    def vertex_normals_set(self):
        """jade_scene_get_vertex_normals: whether the handle carries a table."""
        fn = self._hip_only("jade_scene_get_vertex_normals")
        on = C.c_int(-1)
        self.backend.check(fn(self._h, C.byref(on)))
        return bool(on.value)

    def set_textures(self, images, uv=None, image_of=None):
        """jade_scene_set_textures: images - a list of float32 [height, width, 3] arrays of linear RGB, row 0 at v = 0; uv - float32
        [n_triangles, 3, 2], the (u, v) of the corners p1 p2 p3, triangles in the scene's order; image_of - int32 [n_triangles], each
        triangle's image or -1 for none.  None (or no images) clears.  The next render this handle begins multiplies the image, filtered
        at every path vertex, into the triangle's brdf and refract_albedo (HIP module only; include/jade_bvh.h, "The surface colour,
        stated"); a table in which no triangle names an image is today's render bit for bit."""
        fn = self._hip_only("jade_scene_set_textures")
        if images is None or len(images) == 0:
            self.backend.check(fn(self._h, 0, None, None, None, 0))
            return
        imgs = [np.ascontiguousarray(im, np.float32) for im in images]
        for k, im in enumerate(imgs):
            if im.ndim != 3 or im.shape[2] != 3:
                raise JadeError(_abi.JADE_ERR_INVALID, f"textures: image {k} is not [height, width, 3]")
        arr = (_abi.TextureImage * len(imgs))(*[_abi.TextureImage(im.shape[1], im.shape[0], C.cast(im.ctypes.data, C.POINTER(C.c_float))) for im in imgs])
        u = np.ascontiguousarray(uv, np.float32)
        io = np.ascontiguousarray(image_of, np.int32).reshape(-1)
        if u.size != 6 * io.size:
            raise JadeError(_abi.JADE_ERR_INVALID, "textures: 6 floats of uv and one image number per triangle")
        self.backend.check(fn(self._h, len(imgs), arr, u.ctypes.data, io.ctypes.data, io.size))

    @property
    def textures(self):
        """jade_scene_get_textures: whether the handle carries a texture table."""
        fn = self._hip_only("jade_scene_get_textures")
        on = C.c_int(-1)
        self.backend.check(fn(self._h, C.byref(on)))
        return bool(on.value)

    def set_normal_maps(self, images, uv=None, image_of=None, strength=1.0):
        """jade_scene_set_normal_maps: images - a list of float32 [height, width, 3] arrays of tangent-space vectors (x, y, z), already
        decoded (host.load_normal_map, host.height_to_normal_map), row 0 at v = 0; uv - float32 [n_triangles, 3, 2] and image_of - int32
        [n_triangles], the map's own, -1 for a triangle without a map; strength - finite and >= 0, scales x and y.  None (or no images)
        clears.  The next render this handle begins bends the shading normal of every path vertex on a mapped triangle (HIP module only;
        include/jade_bvh.h, "The mapped normal, stated"); a table that maps no triangle is today's render bit for bit."""
        fn = self._hip_only("jade_scene_set_normal_maps")
        if images is None or len(images) == 0:
            self.backend.check(fn(self._h, 0, None, None, None, 0, 1.0))
            return
        imgs = [np.ascontiguousarray(im, np.float32) for im in images]
        for k, im in enumerate(imgs):
            if im.ndim != 3 or im.shape[2] != 3:
                raise JadeError(_abi.JADE_ERR_INVALID, f"normal maps: image {k} is not [height, width, 3]")
        arr = (_abi.TextureImage * len(imgs))(*[_abi.TextureImage(im.shape[1], im.shape[0], C.cast(im.ctypes.data, C.POINTER(C.c_float))) for im in imgs])
        u = np.ascontiguousarray(uv, np.float32)
        io = np.ascontiguousarray(image_of, np.int32).reshape(-1)
        if u.size != 6 * io.size:
            raise JadeError(_abi.JADE_ERR_INVALID, "normal maps: 6 floats of uv and one image number per triangle")
        self.backend.check(fn(self._h, len(imgs), arr, u.ctypes.data, io.ctypes.data, io.size, float(strength)))

    @property
    def normal_maps(self):
        """jade_scene_get_normal_maps: whether the handle carries a normal-map table."""
        fn = self._hip_only("jade_scene_get_normal_maps")
        on = C.c_int(-1)
        self.backend.check(fn(self._h, C.byref(on)))
        return bool(on.value)

    def set_passes(self, on):
        """jade_scene_set_passes: the next render this handle begins keeps, beside its frame, the same radiance split into the
        _abi.PASS_COUNT light passes (HIP module only; include/jade_bvh.h, "The passes, stated").  The frame does not change in any bit."""
        fn = self._hip_only("jade_scene_set_passes")
        self.backend.check(fn(self._h, 1 if on else 0))

    @property
    def passes_enabled(self):
        """jade_scene_get_passes: whether the next render of this handle keeps passes."""
        fn = self._hip_only("jade_scene_get_passes")
        on = C.c_int(-1)
        self.backend.check(fn(self._h, C.byref(on)))
        return bool(on.value)

    def passes(self):
        """jade_render_passes: the passes of the render in progress over the samples finished so far, a dict from jade_pass_name's names
        (_abi.PASS_NAMES, in index order) to float32 [H, W, 3] arrays laid out as resolve's rgb; tiles this rank does not own are 0."""
        fn = self._hip_only("jade_render_passes")
        if self._params is None:
            raise JadeError(_abi.JADE_ERR_INVALID, "jade_render_begin not called")
        name = self._hip_only("jade_pass_name")
        out = np.zeros((_abi.PASS_COUNT, self._params.height, self._params.width, 3), np.float32)
        self.backend.check(fn(self._h, out.ctypes.data))
        return {name(i).decode(): out[i] for i in range(_abi.PASS_COUNT)}

    def focus_distance(self, params, px, py):
        """jadeh_focus_distance: the depth along the camera's axis of what the centre of pixel (px, py) of the frame `params` shows
        (row 0 = the bottom row) - the focus_distance that puts it in focus.  Traced with this backend's jade_trace_rays; a pixel that
        shows the sky, or lies outside the frame, raises RuntimeError."""
        from . import host
        lib = host.host_lib()
        out = C.c_float(0.0)
        trace = C.cast(self.backend.lib.jade_trace_rays, C.c_void_p)
        if lib.jadeh_focus_distance(trace, self._h, C.byref(params), int(px), int(py), C.byref(out)) != 0:
            raise RuntimeError(lib.jadeh_last_error().decode())
        return out.value

    def meter(self):
        """jade_render_meter: the Meter of the render in progress over the in-image pixels of the owned tiles."""
        fn = self._hip_only("jade_render_meter")
        m = _abi.MeterStruct()
        self.backend.check(fn(self._h, C.byref(m)))
        return Meter.from_struct(m)

    def query(self, what):
        """jade_render_query: what the backend holds for the current render (_abi.Q_*)."""
        v = C.c_int64(0)
        self.backend.check(self.backend.lib.jade_render_query(self._h, int(what), C.byref(v)))
        return v.value

    def resolve_tiles_device(self, dev_ptr, stream=0):
        self.backend.check(self.backend.lib.jade_render_resolve_tiles_device(self._h, C.c_void_p(dev_ptr), C.c_void_p(stream)))

    def trace_rays(self, origins, dirs, skip):
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        s = np.ascontiguousarray(skip, np.int32).reshape(-1)
        n = len(o)
        assert len(d) == n and len(s) == n
        idx = np.zeros(n, np.int32)
        dist = np.zeros(n, np.float32)
        pt = np.zeros((n, 3), np.float32)
        st = _abi.Stats()
        self.backend.check(self.backend.lib.jade_trace_rays(self._h, n, o.ctypes.data, d.ctypes.data, s.ctypes.data,
                                                            idx.ctypes.data, dist.ctypes.data, pt.ctypes.data, C.byref(st)))
        return idx, dist, pt, st


def render_multi(backend, scenes, params, want_rgb=True, want_bgr8=True):
    """jade_render_multi: one frame over several scenes (one per device) from this process."""
    h, w = params.height, params.width
    rgb = np.zeros((h, w, 3), np.float32) if want_rgb else None
    bgr = np.zeros((h, w, 3), np.uint8) if want_bgr8 else None
    st = _abi.Stats()
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    backend.check(backend.lib.jade_render_multi(arr, len(scenes), C.byref(params), rgb.ctypes.data if want_rgb else None,
                                                bgr.ctypes.data if want_bgr8 else None, C.byref(st)))
    return rgb, bgr, st


_hip = None


def hip():
    """The product backend.  Fails loudly if the HIP extension was not built."""
    global _hip
    if _hip is None:
        # JADE_HIP_LIB points development tools at another BUILD of the same HIP library (A/B runs)
        _hip = Backend(os.environ.get("JADE_HIP_LIB", HIP_LIB))
    return _hip


def assemble_tiles(tiles, width, height, rank, nranks, out=None):
    """Scatter one rank's compact tile buffer ([n_owned, 16, 16, 3]) into a full image."""
    ts = _abi.TILE_SIZE
    tx = (width + ts - 1) // ts
    ty = (height + ts - 1) // ts
    if out is None:
        out = np.zeros((height, width, 3), tiles.dtype)
    from .distributed import owned_tile_ids
    ids = owned_tile_ids(width, height, rank, nranks)
    for k, tid in enumerate(ids):
        y0, x0 = (tid // tx) * ts, (tid % tx) * ts
        hh, ww = min(ts, height - y0), min(ts, width - x0)
        out[y0:y0 + hh, x0:x0 + ww] = tiles[k, :hh, :ww]
    return out
