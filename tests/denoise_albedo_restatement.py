"""Not a test: albedo demodulation in a frame's denoise filter (ky_amd/csrc/ky_denoise.hpp, demodulate_pixel / remodulate_pixel; DESIGN.md "Denoise", "Albedo")
restated in NumPy, and the albedo buffer itself (denoise_albedo_kernel, ky_amd/csrc/ky_denoise.hip) restated on the CPU oracle's camera and scene-intersect KATs
with tests/texture_restatement.py's colours.  The levels are tests/denoise_restatement.py's (denoise_chains_restatement.py's where keys are given).
The keyword arguments `variance`, `remodulate_floor` and `swap` name the second variance rule and the defects that tests/test_denoise_albedo.py shows failing."""
import numpy as np

import denoise_chains_restatement as DC
import denoise_restatement as D
import filter_restatement as F
import lens_restatement as L
import texture_restatement as X

f32, f64 = np.float32, np.float64
FLOOR = f32(1.0 / 64.0)
RAY_OFFSET = f32(1e-2)   # K_RAY_OFFSET, offset_ray_origin
MATTE, MIRROR, GLASS, PLASTIC = 0, 1, 2, 3


# ---- the arithmetic around the levels ----

def floored(albedo):
    """a' = max(a, 1/64) per channel of [..., >= 3] float32 -> float64 (a NaN takes the floor)"""
    a = np.asarray(albedo, f32)[..., :3]
    with np.errstate(invalid="ignore"):
        return np.where(a > FLOOR, a, FLOOR).astype(f64)


def luminance64(a):
    return 0.212671 * a[..., 0] + 0.715160 * a[..., 1] + 0.072169 * a[..., 2]


def demodulate(cv, gb, albedo, variance="y2"):
    """demodulate_pixel over the film: class-0 pixels' c <- (float)(c / a'), v <- (float)(v / Y(a')^2).  variance="inv": the second rule, v Y(1 / a')^2;
    variance="none": the named defect `the variance scale forgotten`."""
    ap = floored(albedo)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = (cv[..., :3].astype(f64) / ap).astype(f32)
        if variance == "y2":
            ya = luminance64(ap)
            v = (cv[..., 3].astype(f64) / (ya * ya)).astype(f32)
        elif variance == "inv":
            yi = luminance64(1.0 / ap)
            v = (cv[..., 3].astype(f64) * (yi * yi)).astype(f32)
        else:
            v = cv[..., 3]
    out = np.concatenate([c, v[..., None]], axis=-1).astype(f32)
    return np.where((gb[..., 3] == D.SURFACE)[..., None], out, cv)


def remodulate(cv, gb, albedo, remodulate_floor=True):
    """remodulate_pixel over the film: class-0 pixels' c <- (float)(c a').  remodulate_floor=False: the named defect `remodulated with a instead of a'`."""
    ap = floored(albedo) if remodulate_floor else np.asarray(albedo, f32)[..., :3].astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (cv[..., :3].astype(f64) * ap).astype(f32)
    out = np.concatenate([c, cv[..., 3:4]], axis=-1).astype(f32)
    return np.where((gb[..., 3] == D.SURFACE)[..., None], out, cv)


def denoise(cv, ga, gb, albedo, pix, key=None, levels=D.DEFAULTS["levels"], variance="y2", remodulate_floor=True, **params):
    """demodulate -> the levels (keyed where `key` is given) -> remodulate: [H, W, 4] float32, unclamped"""
    cv = demodulate(cv, gb, albedo, variance)
    cv = D.denoise(cv, ga, gb, pix, levels=levels, **params) if key is None else DC.denoise(cv, ga, gb, key, pix, levels=levels, **params)
    return remodulate(cv, gb, albedo, remodulate_floor)


# ---- the albedo buffer ----

def pairs(G):
    """The G^2 sub-samples in visit order (j-major, i inner): film pairs ((i + 0.5) g, (j + 0.5) g) and lens pairs ((j + 0.5) g, (G - 1 - i + 0.5) g), float32, with
    g the float32 1 / G -> ([G^2, 2], [G^2, 2])"""
    g = f32(1) / f32(G)
    j, i = np.mgrid[0:G, 0:G]
    i, j = i.ravel().astype(f32), j.ravel().astype(f32)
    at = lambda k: ((k + f32(0.5)) * g).astype(f32)
    return np.stack([at(i), at(j)], axis=1), np.stack([at(j), at(f32(G - 1) - i)], axis=1)


def camera_rays(O, camera, w, h, G, flt=None, lens=None, shift=(0.0, 0.0)):
    """The camera rays of every sub-sample of every pixel, [h w G^2, 6] float32, pixel-major in film order.  flt: a filter_restatement.Filter whose warp the film pair
    goes through; lens: (radius, focus) -- the lens pair through lens_restatement's disk and ray.  shift: added to the film point, in pixels (the clean test)."""
    film, lens_pairs = pairs(G)
    if flt is not None and flt.kind != F.BOX:
        film = np.stack([F.warp(flt, film[:, 0]), F.warp(flt, film[:, 1])], axis=1)
    ys, xs = np.mgrid[0:h, 0:w]
    px = (xs.ravel().astype(f32)[:, None] + film[None, :, 0]).astype(f32).ravel()
    py = (ys.ravel().astype(f32)[:, None] + film[None, :, 1]).astype(f32).ravel()
    origin = None
    if lens is not None:
        cam = L.Camera(camera)
        px, py, origin = L.lens_ray(cam, L.lens_const(cam, *lens), px, py, np.tile(L.disk(lens_pairs), (w * h, 1)))
    px, py = (px + f32(shift[0])).astype(f32), (py + f32(shift[1])).astype(f32)
    rays = np.asarray(O.kat_camera(camera, np.stack([px, py], axis=1)), f32)
    if origin is not None:
        rays[:, :3] = origin
    return rays


def scene_c(scene):
    return scene.scene if hasattr(scene, "scene") else scene.c


def surface_colour(A, c, textures, surface, position, swap=False):
    """c0 of the material of each hit (surface [n] caller's index, position [n, 3]) as a vertex there takes it: the texture's colour where the material has one,
    color0 elsewhere, divided by diffuse_probability on plastic -> (colour [n, 3] float32, clean [n]: >= 1e-4 from a cell or texel edge).  swap: the named defect
    `u and v swapped`."""
    by_material = {t.material: t for t in textures}
    colour = np.ones((len(surface), 3), f32)
    clean = np.ones(len(surface), bool)
    for s in np.unique(surface[surface >= 0]):
        rows = surface == s
        m = c.surfaces[int(s)].material
        M = c.materials[m]
        tex = by_material.get(m)
        if tex is None:
            col = np.tile(np.array([M.color0[j] for j in range(3)], f32), (int(rows.sum()), 1))
        else:
            shape = X.Shape.of(c.shapes[c.surfaces[int(s)].shape])
            u, v = X.uv(shape, position[rows], f32, swap)
            us, vs = X.transform(tex, u, v, f32)
            col = X.lookup(tex, us, vs, f32).astype(f32)
            u64, v64 = X.uv(shape, position[rows], f64, swap)
            us64, vs64 = X.transform(tex, u64, v64, f64)
            clean[rows] = X.edge_distance(tex, us64, vs64) >= 1e-4
        if M.kind == PLASTIC:
            col = (col / f32(M.diffuse_probability)).astype(f32)
        colour[rows] = col
    return colour, clean


def walk(O, A, scene, textures, rays, bounces, swap=False):
    """Every ray [n, 6] walked as denoise_albedo_kernel walks a sub-sample, mirrors followed for up to `bounces` vertices -> (colour [n, 3] float32, ended [n] bool: on
    a surface without a lamp, surfaces [n, bounces + 1] the caller's indices along the walk or -1, clean [n], branch [n, bounces + 1]: 1 where glass transmitted).
    Glass walked THROUGH (bounces > 0 only) is bsdf_sample_delta at u = 0.5 restated in double: the Fresnel reflectance F of the unpolarised wave decides -- reflected
    where 0.5 < F, total internal reflection included -- and the branch multiplies by color0 (reflected) or color1 (transmitted); a ray with |F - 0.5| < 0.02 is
    not clean."""
    c = scene_c(scene)
    n = len(rays)
    colour = np.ones((n, 3), f32)
    ended, clean, alive = np.zeros(n, bool), np.ones(n, bool), np.ones(n, bool)
    seq = np.full((n, bounces + 1), -1, np.int64)
    branch = np.zeros((n, bounces + 1), np.int8)
    etas = np.array([c.materials[c.surfaces[s].material].eta for s in range(c.surface_count)], f64)
    c01 = np.array([[list(c.materials[c.surfaces[s].material].color0), list(c.materials[c.surfaces[s].material].color1)] for s in range(c.surface_count)], f32)
    rays = np.array(rays, f32)
    kinds = np.array([c.materials[c.surfaces[s].material].kind for s in range(c.surface_count)])
    lamp = np.array([c.surfaces[s].area_light >= 0 for s in range(c.surface_count)])
    for k in range(bounces + 1):
        idx = np.nonzero(alive)[0]
        if not len(idx):
            break
        hit = O.kat_scene_intersect(scene, np.concatenate([rays[idx], np.full((len(idx), 1), np.inf, f32)], axis=1))
        ok = hit[:, 0] > 0
        s = np.where(ok, hit[:, 8].astype(np.int64), -1)
        seq[idx, k] = s
        alive[idx[~ok]] = False
        on = ok & ~lamp[np.maximum(s, 0)]
        alive[idx[ok & ~on]] = False                      # a lamp: multiplies by nothing, is not counted
        kind = kinds[np.maximum(s, 0)]
        col, cl = surface_colour(A, c, textures, np.where(on, s, -1), hit[:, 2:5], swap)
        last = k == bounces
        ends = on & ((kind == MATTE) | (kind == PLASTIC) | last)
        takes = on & (kind != GLASS)                      # every surface but glass multiplies by its c0, where the walk ends and where it goes on
        colour[idx[takes]] = (colour[idx[takes]] * col[takes]).astype(f32)
        clean[idx[takes]] &= cl[takes]
        ended[idx[ends]] = True
        alive[idx[ends]] = False
        tg = on & ~ends & (kind == GLASS)
        if tg.any():
            rows = idx[tg]
            d, nrm, p = rays[rows, 3:6].astype(f64), hit[tg, 5:8].astype(f64), hit[tg, 2:5].astype(f64)
            wo = -d
            cos_o = np.sum(nrm * wo, axis=1)
            into = cos_o > 0
            eta = etas[s[tg]]
            ratio = np.where(into, 1.0 / eta, eta)
            ei, et = np.where(into, 1.0, eta), np.where(into, eta, 1.0)
            ci = np.minimum(np.abs(cos_o), 1.0)
            st = ratio * np.sqrt(np.maximum(0.0, 1.0 - ci * ci))
            ct = np.sqrt(np.maximum(0.0, 1.0 - st * st))
            r_para = (et * ci - ei * ct) / (et * ci + ei * ct)
            r_perp = (ei * ci - et * ct) / (ei * ci + et * ct)
            F_ = np.where(st >= 1.0, 1.0, 0.5 * (r_para * r_para + r_perp * r_perp))
            refl = 0.5 < F_
            clean[rows] &= np.abs(F_ - 0.5) >= 0.02
            kk = ratio * ci - ct
            nz = np.where(into, 1.0, -1.0)
            wi = np.where(refl[:, None], -wo + 2.0 * cos_o[:, None] * nrm, wo * (-ratio)[:, None] + nrm * (kk * nz)[:, None])
            colour[rows] = (colour[rows] * c01[s[tg], np.where(refl, 0, 1)]).astype(f32)
            branch[rows, k] = np.where(refl, 0, 1)
            side = np.where(np.sum(nrm * wi, axis=1, keepdims=True) < 0, -1.0, 1.0)
            rays[rows, :3] = (p + nrm * side * float(RAY_OFFSET)).astype(f32)
            rays[rows, 3:6] = wi.astype(f32)
        go = on & ~ends & (kind == MIRROR)
        if go.any():
            d, nrm, p = rays[idx[go], 3:6].astype(f64), hit[go, 5:8].astype(f64), hit[go, 2:5].astype(f64)
            wi = d - 2.0 * np.sum(d * nrm, axis=1, keepdims=True) * nrm
            side = np.where(np.sum(nrm * wi, axis=1, keepdims=True) < 0, -1.0, 1.0)
            rays[idx[go], :3] = (p + nrm * side * float(RAY_OFFSET)).astype(f32)
            rays[idx[go], 3:6] = wi.astype(f32)
    return colour, ended, seq, clean, branch


def albedo(O, A, scene, textures, w, h, G, bounces=0, flt=None, lens=None, swap=False, check_clean=True):
    """The albedo buffer restated: ([h, w, 4] float32 {r, g, b, count}, clean [h, w], first-hit surfaces [h, w, G^2]).  A pixel is clean when every sub-sample is >= 1e-4 from a cell or texel edge,
    and the surfaces and glass branches along its walk do not change when the film point moves by +-1e-3 pixel along either axis."""
    c = scene_c(scene)
    colour, ended, seq, clean, branch = walk(O, A, scene, textures, camera_rays(O, c.camera, w, h, G, flt, lens), bounces, swap)
    if check_clean:
        for shift in ((1e-3, 0.0), (-1e-3, 0.0), (0.0, 1e-3), (0.0, -1e-3)):
            moved = walk(O, A, scene, textures, camera_rays(O, c.camera, w, h, G, flt, lens, shift), bounces, swap)
            clean &= (moved[2] == seq).all(axis=1) & (moved[4] == branch).all(axis=1)
    colour = colour.reshape(h * w, G * G, 3)
    total = np.zeros((h * w, 3), f32)
    for k in range(G * G):   # float32, in visit order
        total = (total + colour[:, k]).astype(f32)
    out = np.concatenate([(total * (f32(1) / f32(G * G))).astype(f32), ended.reshape(h * w, G * G).sum(axis=1).astype(f32)[:, None]], axis=1)
    first = seq[:, 0].reshape(h * w, G * G)
    return out.reshape(h, w, 4), clean.reshape(h * w, G * G).all(axis=1).reshape(h, w), first.reshape(h, w, G * G)


# ---- a frame in passes replayed on the oracle (tools/denoise_replay.py albedo; tests/test_denoise_albedo.py) ----

def replay(O, api, R, scene, w, h, spp, seed, at):
    """The frame (w x h, spp samples in all, one chunk per pass) replayed on the oracle's per-sample radiance of `scene` up to the largest count in `at`:
    {samples done: the gather's [h, w, 4] float32 {r, g, b, v} at that pass boundary}.  R: tests/noise_restatement.py."""
    upto = max(at)
    p = api.make_params(w, h, spp, seed=seed)
    rad = np.stack([O.li(scene, p, i % w, i // w, 0, upto).astype(f64) for i in range(w * h)])   # [pixel (film order), sample, 3]
    cum = np.cumsum(rad, axis=1)
    y_prev, m2, n_prev = np.zeros(w * h), np.zeros(w * h), 0
    out = {}
    for k, d in enumerate(api.pass_boundaries(spp)):
        if d > upto:
            break
        accum = np.rint(cum[:, d - 1] / spp * 4294967296.0).astype(np.int64)
        y_prev, m2 = R.update(y_prev, m2, R.luminance(accum, spp), n_prev, d)
        n_prev = d
        if d in at:
            out[d] = D.gather(accum, np.zeros(w * h, np.uint32), m2, spp, d, k + 1).reshape(h, w, 4)
    return out


def rmse(film, truth, sel):
    return float(np.sqrt((((np.clip(film[..., :3].astype(f64), 0, 1) - truth) ** 2)[sel]).mean()))
