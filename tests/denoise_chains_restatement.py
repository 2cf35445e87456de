"""The denoiser's specular-chain guides (include/kyhip.h, kyhip_frame_set_guide_bounces; DESIGN.md "Denoise", "Guides beyond the first hit") restated in NumPy:
the keyed a-trous level (ky_amd/csrc/ky_denoise.hpp, level_pixel_t<true>: a pixel's taps and its variance prefilter's neighbours are the class-0 pixels with the
SAME chain key -- tests/denoise_restatement.py's level with that one condition more), and the chain walk itself fed with the rows of a per-vertex trace
(api.kat_li_trace or the oracle's trace_li under the debug sampler: 26 floats per path vertex).  Shared by tests/test_denoise_chains.py,
tests/test_denoise_chains_gpu.py, tests/golden/make_denoise_chains.py and tools/denoise_replay.py."""
import numpy as np

import denoise_restatement as D

F64 = np.float64
MAX_BOUNCES = 4
DIGIT_BITS = 10
UNRESOLVED = 1 << 62
RAY_OFFSET = 1e-2      # offset_ray_origin
LOBE_MIRROR, LOBE_GLASS = 1, 2
BSDF_TRANSMISSION = 2
# a trace row: bounces, surface, lobe, P[3], n[3], wo[3], beta[3], Lo[3], f[3], pdf, |cos|, flags, decisions[2]
R_SURFACE, R_LOBE, R_P, R_N, R_WO, R_FLAGS = 1, 2, slice(3, 6), slice(6, 9), slice(9, 12), 23


def level(cv, ga, gb, key, step, pix, normal_squarings=D.DEFAULTS["normal_squarings"], sigma_luminance=D.DEFAULTS["sigma_luminance"],
          sigma_plane=D.DEFAULTS["sigma_plane"], **_):
    """level_pixel_t<true> over the film: D.level, operation by operation, with `key_q == key_p` among the conditions of a tap and of a prefilter neighbour."""
    surface = gb[..., 3] == D.SURFACE
    key = np.asarray(key, np.uint64)
    sigma_l2 = float(np.float32(sigma_luminance)) * float(np.float32(sigma_luminance))
    sigma_p = float(np.float32(sigma_plane))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        vw, vs = np.zeros(surface.shape, F64), np.zeros(surface.shape, F64)
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                (vq, ok), (sq, _), (kq, _) = D._tap(cv[..., 3], i, j), D._tap(surface, i, j), D._tap(key, i, j)
                ok = ok & sq & (kq == key)
                h = D.TAP3[abs(i)] * D.TAP3[abs(j)]
                vw = vw + np.where(ok, h, 0.0)
                vs = vs + np.where(ok, h * vq.astype(F64), 0.0)
        v_bar = vs / vw
        lum_den = sigma_l2 * v_bar + 1e-10
        plane_den = np.maximum(sigma_p * ga[..., 3].astype(F64) * pix * float(step), 1e-300)
        yp = D.luminance(cv)
        n_p, p_p = ga[..., :3].astype(F64), gb[..., :3].astype(F64)
        sw = np.zeros(surface.shape, F64)
        sums = [np.zeros(surface.shape, F64) for _ in range(4)]
        for j in (-2, -1, 0, 1, 2):
            for i in (-2, -1, 0, 1, 2):
                (cq, ok), (aq, _), (bq, _), (sq, _), (kq, _) = (D._tap(a, i * step, j * step) for a in (cv, ga, gb, surface, key))
                ok = ok & sq & (kq == key)
                n_q, p_q = aq[..., :3].astype(F64), bq[..., :3].astype(F64)
                nd = n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1] + n_p[..., 2] * n_q[..., 2]
                wn = np.where(nd > 0.0, nd, 0.0)
                for _s in range(normal_squarings):
                    wn = wn * wn
                d = p_q - p_p
                xp = (n_p[..., 0] * d[..., 0] + n_p[..., 1] * d[..., 1] + n_p[..., 2] * d[..., 2]) / plane_den
                pa = 1.0 + xp * xp
                wp = 1.0 / (pa * pa)
                dl = yp - D.luminance(cq)
                la = 1.0 + dl * dl / lum_den
                wl = 1.0 / (la * la)
                w = np.where(ok, D.TAP5[abs(i)] * D.TAP5[abs(j)] * wn * wp * wl, 0.0)
                sw = sw + w
                for ch in range(3):
                    sums[ch] = sums[ch] + np.where(ok, w * cq[..., ch].astype(F64), 0.0)
                sums[3] = sums[3] + np.where(ok, w * w * cq[..., 3].astype(F64), 0.0)
        new = np.stack([sums[0] / sw, sums[1] / sw, sums[2] / sw, sums[3] / (sw * sw)], axis=-1).astype(np.float32)
    return np.where(surface[..., None], new, cv)


def denoise(cv, ga, gb, key, pix, levels=D.DEFAULTS["levels"], **params):
    """The keyed filter: `levels` levels with steps 1, 2, 4 ... -> the last level's [H, W, 4] float32, unclamped."""
    for k in range(levels):
        cv = level(cv, ga, gb, key, 1 << k, pix, **params)
    return cv


def digit(surface, transmitted):
    return ((int(surface) + 1) << 1) | (1 if transmitted else 0)


def chain(rows, scene_c, bounces):
    """The chain walk of one pixel (include/kyhip.h) on the rows of its centre sample's per-vertex trace under the debug sampler (row k: the path's k-th vertex)
    -> (class, key, ga[4], gb[4]) in float64.  A chain vertex the trace has no row for is a ray that left the scene.  t is not part of a row: it is the distance
    from the ray's origin -- the camera, or the previous vertex moved RAY_OFFSET along its normal to the side the path leaves to -- to the vertex."""
    cam = np.array([scene_c.camera.position[i] for i in range(3)], F64)
    rows = np.asarray(rows, F64)
    key, t_sum, origin, first = 0, 0.0, cam, None
    for k in range(bounces + 1):
        if k >= len(rows):
            return D.MISS, key, np.zeros(4), np.array([0.0, 0.0, 0.0, D.MISS])
        r = rows[k]
        P, n = r[R_P], r[R_N]
        t_sum += float(np.linalg.norm(P - origin))
        light = scene_c.surfaces[int(r[R_SURFACE])].area_light >= 0
        here = (np.concatenate([n, [t_sum]]), np.concatenate([P, [D.LIGHT if light else D.SURFACE]]))
        if k == 0:
            first = here
        if light:
            return D.LIGHT, key, here[0], here[1]
        if int(r[R_LOBE]) not in (LOBE_MIRROR, LOBE_GLASS):
            return D.SURFACE, key, here[0], here[1]
        if k == bounces:
            return D.SURFACE, UNRESOLVED | (key & ((1 << DIGIT_BITS) - 1)), first[0], first[1]
        key |= digit(r[R_SURFACE], int(r[R_FLAGS]) & BSDF_TRANSMISSION) << (DIGIT_BITS * k)
        if k + 1 < len(rows):
            wi = -rows[k + 1][R_WO]
            origin = P + n * (RAY_OFFSET if float(n @ wi) >= 0 else -RAY_OFFSET)
    raise AssertionError("unreachable: the turn with k == bounces returns")


def chains(trace, scene_c, w, h, bounces):
    """chain() over the film: trace(x, y) -> the rows of pixel (x, y)'s centre sample.  -> (class [h, w], key [h, w] uint64, ga, gb [h, w, 4] float32)."""
    cls, key = np.zeros((h, w), np.float32), np.zeros((h, w), np.uint64)
    ga, gb = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    for y in range(h):
        for x in range(w):
            c, k, a, b = chain(trace(x, y), scene_c, bounces)
            cls[y, x], key[y, x], ga[y, x], gb[y, x] = c, k, a, b
    return cls, key, ga, gb


def counts(cls, key):
    """(pixels whose key is not 0, those of them that end on a surface or a lamp, those that leave the scene, the distinct keys among them)."""
    chained = key != 0
    return int(chained.sum()), int((chained & (cls != D.MISS)).sum()), int((chained & (cls == D.MISS)).sum()), len(np.unique(key[chained]))
