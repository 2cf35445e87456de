"""The thin lens (include/kyhip.h, ky_lens) restated in NumPy, independently of ky_amd/csrc: Shirley's concentric map of the square onto the
disk, the launch constants as the host rounds them, the shifted film point and origin of a lens ray exactly as section 12 writes them, and the tape and camera
position that make the CPU oracle -- a pinhole camera -- trace a lens sample: kyo_li_tape adds a row's first two numbers to the pixel's corner whatever they are,
and a pinhole at the lens point sends the ray of the shifted film point through the pinhole ray's point on the focus plane.
Not a test: tests/test_lens.py and tests/test_lens_gpu.py import it."""
import ctypes as C
import math

import numpy as np

import filter_restatement as F

f32 = np.float32
f64 = np.float64
QUARTER_PI = f32(0.78539816339744830962)


def disk(u2, dtype=f32):
    """[n, 2] numbers in [0, 1)^2 -> [n, 2] points of the unit disk.  (a, b) = 2 u - 1; the longer of the two is the radius r, the shorter over the longer is q,
    t = (pi / 4) q the angle from the wedge's axis, and the point is r (cos t, sin t) where |a| > |b|, r (sin t, cos t) elsewhere -- cos(pi / 2 - t) = sin t.
    dtype float32: every product, difference and quotient rounded once to float32 as the device rounds them (its quotient is not correctly rounded: the GPU test
    measures what that costs), sine and cosine in double and rounded once.  dtype float64: the same map of the same float32 inputs in double throughout."""
    u2 = np.asarray(u2, f32).reshape(-1, 2)
    a = (dtype(2) * u2[:, 0].astype(dtype) - dtype(1)).astype(dtype)
    b = (dtype(2) * u2[:, 1].astype(dtype) - dtype(1)).astype(dtype)
    wide = np.abs(a) > np.abs(b)
    r = np.where(wide, a, b)
    num = np.where(wide, b, a)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(r == 0, dtype(0), (num / r).astype(dtype)).astype(dtype)
    t = ((QUARTER_PI if dtype is f32 else f64(math.pi / 4)) * q).astype(dtype)
    c = (r * np.cos(t.astype(f64)).astype(dtype)).astype(dtype)
    s = (r * np.sin(t.astype(f64)).astype(dtype)).astype(dtype)
    return np.stack([np.where(wide, c, s), np.where(wide, s, c)], axis=1).astype(dtype)


class Camera:
    """A ky_camera's vectors as float32 arrays."""

    def __init__(self, cam):
        self.position = np.array(list(cam.position), f32)
        self.front = np.array(list(cam.front), f32)
        self.right = np.array(list(cam.right), f32)
        self.up = np.array(list(cam.up), f32)
        self.resolution = np.array(list(cam.resolution), f32)


def lens_const(cam, radius, focus):
    """(ar, bu, wf, hf) float32: radius / |right|, radius / |up|, w |front| / focus, h |front| / focus, in double from the float32 camera, rounded once."""
    n = lambda v: math.sqrt(float(np.dot(v.astype(f64), v.astype(f64))))
    radius, focus = float(f32(radius)), float(f32(focus))
    t = n(cam.front) / focus
    return f32(radius / n(cam.right)), f32(radius / n(cam.up)), f32(float(cam.resolution[0]) * t), f32(float(cam.resolution[1]) * t)


def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in double; the sum is rounded to 53 bits, then to 24 (filter_restatement.warp's note on the double rounding)."""
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def lens_ray(cam, lc, px, py, d2, sign=1.0):
    """The film point and origin of the lens ray of film point (px, py) (float32 arrays) and disk point d2 [n, 2]: (px', py', origin [n, 3]).
        a = ar dx, b = bu dy;  px' = px - a wf;  py' = py + b hf;  origin = position + right a + up b
    each line one float32 product or fused multiply-add.  sign = -1 is the named defect `the film point shifted with the wrong sign`, which tests/test_lens.py
    must reject."""
    ar, bu, wf, hf = lc
    d2 = np.asarray(d2, f32).reshape(-1, 2)
    a = (ar * d2[:, 0]).astype(f32)
    b = (bu * d2[:, 1]).astype(f32)
    s = f32(sign)
    px2 = fma32(-a * s, wf, px)
    py2 = fma32(b * s, hf, py)
    o = np.stack([fma32(cam.up[k], b, fma32(cam.right[k], a, np.full(a.shape, cam.position[k], f32))) for k in range(3)], axis=1)
    return px2, py2, o


def sample_rows(cam, lc, seed, pixel_key, x, y, n_spp, stride, sampler, flt=None, tab=None):
    """What the oracle needs to trace the n_spp lens samples of pixel (x, y): (rows [N, stride] float32, origins [N, 3] float32).  Row i is the tape of sample i --
    the shifted film point's offsets from the pixel's corner, then the draws after the lens pair -- and origins[i] its lens point, the camera position to give the
    oracle for that sample.  The sample's numbers are filter_restatement.tape's (the random or the stratified stream, the camera pair warped by `flt`): numbers 0
    and 1 the camera sample, 2 and 3 the lens pair, the path's from 4 on."""
    raw = F.tape(seed, pixel_key, n_spp, stride + 2, sampler, flt, tab)
    px = (f32(x) + raw[:, 0]).astype(f32)
    py = (f32(y) + raw[:, 1]).astype(f32)
    px2, py2, o = lens_ray(cam, lc, px, py, disk(raw[:, 2:4]))
    rows = np.empty((n_spp, stride), f32)
    rows[:, 0] = px2 - f32(x)
    rows[:, 1] = py2 - f32(y)
    rows[:, 2:] = raw[:, 4:]
    return rows, o


class OracleLens:
    """kyo_li_tape once per sample, each through a copy of the scene whose camera stands at that sample's lens point."""

    def __init__(self, O, A, scene, params):
        self.lib = O.load()
        self.lib.kyo_li_tape.argtypes = [A.SP, A.PP, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        flat = scene.flat if hasattr(scene, "flat") else scene
        self.scene = A.Scene.from_buffer_copy(flat.contents)   # (its arrays are the caller's: `scene` must outlive this)
        self.keep = scene
        self.params = params
        self.used = np.zeros(1, np.int32)

    def pixel(self, x, y, rows, origins):
        """[N, 3] float32: the oracle's radiance of each row's sample."""
        rows = np.ascontiguousarray(rows, f32)
        n, stride = rows.shape
        out = np.zeros((n, 3), f32)
        pos = self.scene.camera.position
        for i in range(n):
            pos[0], pos[1], pos[2] = float(origins[i, 0]), float(origins[i, 1]), float(origins[i, 2])
            rc = self.lib.kyo_li_tape(C.byref(self.scene), C.byref(self.params), x, y, rows[i].ctypes.data, stride, 1, out[i].ctypes.data, self.used.ctypes.data)
            if rc != 0:
                raise ValueError("kyo_li_tape returned %d (-2: the sample needed more than %d numbers)" % (rc, stride))
        return out
