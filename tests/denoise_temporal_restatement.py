"""The temporal step of a frame's denoise filter (ky_amd/csrc/ky_denoise.hpp, temporal_pixel_t; DESIGN.md "Denoise", "Temporal") restated in NumPy float64,
operation by operation in the header's order: a class-0 pixel's guide position projected through the HISTORY's camera, the up to four history pixels around the
landing point as taps, and the blend by sample counts.  What the step hands on is float32, as in the header.  The `defect` argument injects one named mistake at a
time (tests/test_denoise_temporal.py shows each failing the test that defines it).  Shared by tests/test_denoise_temporal.py (against the host build of the
header), tests/test_denoise_temporal_gpu.py (against the kernels) and tools/denoise_replay.py temporal."""
import numpy as np

import denoise_albedo_restatement as DA
import denoise_chains_restatement as DC
import denoise_restatement as D

F64 = np.float64
DEFAULTS = dict(max_history=8.0, sigma_plane=0.25, min_weight=0.05, normal_squarings=7)
DEFECTS = ("sy_not_flipped", "no_half", "alpha_swapped", "v_by_w", "m_uncapped")


def camera_vectors(camera):
    """(o', f', r', u') of a ky_camera as float64 triples of its float32 members."""
    return tuple(np.array([float(np.float32(v[i])) for i in range(3)], F64) for v in (camera.position, camera.front, camera.right, camera.up))


def _dot(a, v):
    return a[..., 0] * v[0] + a[..., 1] * v[1] + a[..., 2] * v[2]


def project(P, then, w, h, defect=None):
    """(sx, sy, z) of the points P [..., 3] (float32) on the film of the camera `then` = (o', f', r', u'): pixel (i, j)'s centre is at sx = i, sy = j."""
    o, f, r, u = then
    d = np.stack([P[..., i].astype(F64) - o[i] for i in range(3)], axis=-1)
    z = _dot(d, f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = _dot(d, r) / (r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        b = _dot(d, u) / (u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
        half = 0.0 if defect == "no_half" else 0.5
        sx = float(w) * (0.5 + a / z) - half
        sy = float(h) * ((0.5 + b / z) if defect == "sy_not_flipped" else (0.5 - b / z)) - half
    return sx, sy, z


def temporal(cv, ga, gb, key, hist, n_p, pix, then, max_history=DEFAULTS["max_history"], sigma_plane=DEFAULTS["sigma_plane"], min_weight=DEFAULTS["min_weight"],
             normal_squarings=DEFAULTS["normal_squarings"], defect=None, **_):
    """temporal_pixel_t over the film.  cv, ga, gb [H, W, 4] float32 of the current frame, key [H, W] uint64 or None, hist = None (a history that holds no
    picture) or (hcv, hga, hgb) with hgb = {P, m}; n_p the samples the frame holds; `then` = camera_vectors(the history's camera).
    -> (the history's new cv [H, W, 4], its new gb = {P, m} [H, W, 4], took [H, W] bool: the pixels that took history), float32."""
    assert defect is None or defect in DEFECTS
    h, w = cv.shape[:2]
    n_p = float(n_p)
    surface = gb[..., 3] == D.SURFACE
    eligible = surface if key is None else surface & (np.asarray(key) == 0)
    new_gb = gb.copy()
    new_gb[..., 3] = np.where(eligible, np.float32(n_p), np.float32(0.0))
    if hist is None:
        return cv.copy(), new_gb, np.zeros((h, w), bool)
    hcv, hga, hgb = hist
    max_history, sigma_p, min_weight = (float(np.float32(v)) for v in (max_history, sigma_plane, min_weight))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        sx, sy, z = project(gb[..., :3], then, w, h, defect)
        inside = (z > 0.0) & (sx > -1.0) & (sx < float(w)) & (sy > -1.0) & (sy < float(h))
        sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
        fi, fj = np.floor(sx), np.floor(sy)
        fx, fy = sx - fi, sy - fj
        i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
        plane_den = np.maximum(sigma_p * ga[..., 3].astype(F64) * pix, 1e-300)
        n_pp, p_p = ga[..., :3].astype(F64), gb[..., :3].astype(F64)
        sw = np.zeros((h, w), F64)
        sums = [np.zeros((h, w), F64) for _ in range(5)]
        for dj in (0, 1):
            for di in (0, 1):
                qx, qy = i0 + di, j0 + dj
                ok = inside & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                cq, aq, bq = hcv[cy, cx], hga[cy, cx], hgb[cy, cx]
                ok = ok & (bq[..., 3] > 0)
                hh = (fx if di else 1.0 - fx) * (fy if dj else 1.0 - fy)
                n_q, p_q = aq[..., :3].astype(F64), bq[..., :3].astype(F64)
                nd = n_pp[..., 0] * n_q[..., 0] + n_pp[..., 1] * n_q[..., 1] + n_pp[..., 2] * n_q[..., 2]
                wn = np.where(nd > 0.0, nd, 0.0)
                for _s in range(normal_squarings):
                    wn = wn * wn
                e = p_q - p_p
                xp = (n_pp[..., 0] * e[..., 0] + n_pp[..., 1] * e[..., 1] + n_pp[..., 2] * e[..., 2]) / plane_den
                pa = 1.0 + xp * xp
                wp = 1.0 / (pa * pa)
                wt = np.where(ok, hh * wn * wp, 0.0)
                sw = sw + wt
                for ch in range(3):
                    sums[ch] = sums[ch] + np.where(ok, wt * cq[..., ch].astype(F64), 0.0)
                sums[3] = sums[3] + np.where(ok, (wt if defect == "v_by_w" else wt * wt) * cq[..., 3].astype(F64), 0.0)
                sums[4] = sums[4] + np.where(ok, wt * bq[..., 3].astype(F64), 0.0)
        took = eligible & inside & (sw > 0.0) & (sw >= min_weight)
        m_h = sums[4] / sw
        M = m_h if defect == "m_uncapped" else np.minimum(m_h, max_history * n_p)
        alpha = n_p / (n_p + M)
        beta = 1.0 - alpha
        if defect == "alpha_swapped":
            alpha, beta = beta, alpha
        c_p = cv.astype(F64)
        v_h = sums[3] / sw if defect == "v_by_w" else sums[3] / (sw * sw)
        blended = np.stack([alpha * c_p[..., 0] + beta * (sums[0] / sw), alpha * c_p[..., 1] + beta * (sums[1] / sw), alpha * c_p[..., 2] + beta * (sums[2] / sw),
                            alpha * alpha * c_p[..., 3] + beta * beta * v_h], axis=-1).astype(np.float32)
        m_new = (n_p + M).astype(np.float32)
    new_cv = np.where(took[..., None], blended, cv)
    new_gb[..., 3] = np.where(took, m_new, new_gb[..., 3])
    return new_cv, new_gb, took


def levels(cv, ga, gb, key, albedo, pix, **params):
    """The levels behind the temporal step and the remodulation of a frame with an albedo: tests/denoise_chains_restatement.py's keyed level where key is given,
    tests/denoise_restatement.py's else -> [H, W, 4] float32, unclamped."""
    out = DC.denoise(cv, ga, gb, key, pix, **params) if key is not None else D.denoise(cv, ga, gb, pix, **params)
    return out if albedo is None else DA.remodulate(out, gb, albedo)


# ---- the camera path of the replay, the GPU tests and the driver's like ----
PATH_FRAMES, PATH_SPP, PATH_SEED = 6, 16, 1234     # tools/denoise_replay.py temporal and tests/test_denoise_temporal_gpu.py::test_it_denoises: frame k has seed PATH_SEED + k
PATH_DOLLY, PATH_SIDE, PATH_PAN = 0.6, 0.3, 0.12   # over the whole path: forwards and sideways in scene units, and the pan as the tangent of its angle


PATH_TILT = 0.3                                    # the "lamp out of view" path looks down by this tangent, on all of its frames


def path_camera(A, cam, s, tilt=0.0):
    """The camera at the fraction s = 0 .. 1 of the path from `cam`: dollied forwards by PATH_DOLLY s, moved along its right axis by PATH_SIDE s, panned by
    PATH_PAN s towards its right and, on every frame alike, tilted down by `tilt` (tests/screen_cull_scenes.py's camera_like: the field of view and the aspect stay)"""
    from screen_cull_scenes import camera_like, _unit
    p, f, r, u = (np.array([float(v[0]), float(v[1]), float(v[2])], F64) for v in (cam.position, cam.front, cam.right, cam.up))
    f, r, u = _unit(f), _unit(r), _unit(u)
    return camera_like(A, cam, p + PATH_DOLLY * s * f + PATH_SIDE * s * r, f + PATH_PAN * s * r - tilt * u, u)


class History:
    """kyhip_history restated: what a sequence of temporal calls leaves.  step(...) is one kyhip_frame_denoise_temporal up to the clamp: it takes the gather's cv
    (demodulated already where the frame has an albedo), the frame's guides, key and camera, and returns the filtered [H, W, 4] float32."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.hist, self.then, self.frames = None, None, 0

    def step(self, cv, ga, gb, key, camera, width, n_p, denoise_params, temporal_params=None, albedo=None, defect=None):
        pix = D.pixel_width(camera, width)
        t = dict(DEFAULTS, **(temporal_params or {}))
        new_cv, new_gb, took = temporal(cv, ga, gb, key, self.hist, n_p, pix, self.then, defect=defect, **t)
        self.hist, self.then, self.frames = (new_cv, ga.copy(), new_gb), camera_vectors(camera), self.frames + 1
        self.took = took
        return levels(new_cv, ga, gb, key, albedo, pix, **denoise_params)

    def read(self):
        return self.hist[0], self.hist[2][..., 3]
