"""The glare of include/jade_bvh.h stated in numpy: float64 by default, `dtype=np.float32` to evaluate the same statement in the
device's number format, operation for operation: every product and every sum rounded to dtype, every 1-D sum begun with its first
product and added in the header's order, the weights computed as the library's host code computes them.

The statement is a class, one method per step of the header, so that tests/test_glare_cpu.py can state a mistake as a subclass
that overrides one method; the module-level names (glare, weights, reduce, expand, ...) are the methods of the one true instance."""
import math

import numpy as np

H5 = (1.0 / 16.0, 4.0 / 16.0, 6.0 / 16.0, 4.0 / 16.0, 1.0 / 16.0)  # exact in either format
TOL = 1e-5  # relative L2 of the device against the float64 statement (tests/test_gpu_glare.py says where it comes from)


def level_sizes(h, w, levels):
    """[(H_0, W_0), ..., (H_levels, W_levels)]: W_{k+1} = ceil(W_k / 2); a 1x1 level stays 1x1."""
    out = [(h, w)]
    for _ in range(levels):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


class Statement:
    def weights(self, levels, falloff):
        """w_k = f^(k-1) / sum_j f^(j-1), k = 1 .. levels, in double, as the library's gl_run: every power is f^(k - k0) with k0 =
        levels for f > 1 (relative to the largest, so none overflows) and 1 otherwise, the sum added in increasing k, each power
        divided by it.  `falloff` is taken as given: pass a float32 value for the library's weights."""
        f = float(falloff)
        k0 = levels if f > 1.0 else 1
        p = [math.pow(f, float(k - k0)) for k in range(1, levels + 1)]
        total = 0.0
        for v in p:
            total += v
        return np.array([v / total for v in p], np.float64)

    def add(self, terms, dt):
        """A 1-D sum: the first product, then the others added in the order given, each sum rounded to dt."""
        acc = terms[0]
        for t in terms[1:]:
            acc = (acc + t).astype(dt)
        return acc

    def reduce_source(self, x, i, n):
        """clamp(2x + i) on a level of n entries"""
        return np.clip(2 * x + i, 0, n - 1)

    def reduce1(self, a, axis, dt):
        """REDUCE along one axis: out(x) = sum_i h(i) a(clamp(2x + i)), i = -2 .. 2 added in increasing i."""
        a = np.moveaxis(a, axis, 0)
        n = a.shape[0]
        x = np.arange((n + 1) // 2)
        terms = [(dt(H5[i + 2]) * a[self.reduce_source(x, i, n)]).astype(dt) for i in range(-2, 3)]
        return np.moveaxis(self.add(terms, dt), 0, axis)

    def reduce(self, a, dt=np.float64):
        """L_k -> L_{k+1}: rows (x, axis 1) first, then columns (y, axis 0)."""
        return self.reduce1(self.reduce1(a, 1, dt), 0, dt)

    def expand_sources(self, x, m):
        """(j-1, j, j+1) of fine index x, j = x // 2, clamped to [0, m-1]"""
        j = x // 2
        return np.clip(j - 1, 0, m - 1), np.clip(j, 0, m - 1), np.clip(j + 1, 0, m - 1)

    def expand1(self, a, n, axis, dt):
        """EXPAND along one axis to n entries; source indices clamped to [0, m-1]."""
        a = np.moveaxis(a, axis, 0)
        m = a.shape[0]
        x = np.arange(n)
        lo, mid, hi = (a[i] for i in self.expand_sources(x, m))
        even = self.add([(dt(0.125) * lo).astype(dt), (dt(0.75) * mid).astype(dt), (dt(0.125) * hi).astype(dt)], dt)
        odd = self.add([(dt(0.5) * mid).astype(dt), (dt(0.5) * hi).astype(dt)], dt)
        sel = (x % 2 == 0).reshape((n,) + (1,) * (a.ndim - 1))
        return np.moveaxis(np.where(sel, even, odd), 0, axis)

    def expand(self, a, h, w, dt=np.float64):
        """To h x w: rows (y, axis 0) first, then columns (x, axis 1)."""
        return self.expand1(self.expand1(a, h, 0, dt), w, 1, dt)

    def one_minus(self, strength):
        """(s, 1 - s) as the library holds them: s the caller's float, 1 - s one float subtraction"""
        s = np.float32(strength)
        return s, np.float32(1.0) - s

    def glare(self, rgb, levels=6, strength=0.1, falloff=0.5, dtype=np.float64):
        """out_rgb of jade_glare_image for rgb [H, W, 3], in `dtype`."""
        dt = dtype
        rgb = np.asarray(rgb)
        if strength == 0:
            return rgb.copy()
        bad = ~np.isfinite(rgb).all(-1)
        L = [np.where(bad[..., None], 0, rgb).astype(dt)]
        for _ in range(levels):
            L.append(self.reduce(L[-1], dt))
        w = self.weights(levels, falloff)
        A = (dt(w[levels - 1]) * L[levels]).astype(dt)
        for k in range(levels - 1, 0, -1):
            h, wd = L[k].shape[:2]
            A = ((dt(w[k - 1]) * L[k]).astype(dt) + self.expand(A, h, wd, dt)).astype(dt)
        h, wd = rgb.shape[:2]
        s, one_minus_s = self.one_minus(strength)
        out = ((dt(one_minus_s) * L[0]).astype(dt) + (dt(s) * self.expand(A, h, wd, dt)).astype(dt)).astype(dt)
        return np.where(bad[..., None], rgb, out)


STATEMENT = Statement()
weights, reduce1, reduce, expand1, expand, glare = (STATEMENT.weights, STATEMENT.reduce1, STATEMENT.reduce, STATEMENT.expand1,
                                                    STATEMENT.expand, STATEMENT.glare)
