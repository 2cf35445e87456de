"""sample_single_light's pick by power (direct_sample 113) and by position at the vertex (177) restated in NumPy from the written definition (DESIGN.md section 3,
"One light per vertex"; include/kyhip.h at KY_DIRECT_PICK_POWER): the emitter proxies and the power rule's probabilities as the host makes them, the spatial
rule's weights, and the one-pass selection -- operation for operation what ky_pack.cpp's pack_light_pick and ky_device.hpp's pick_light do, in fp32 (or, with
T = np.float64, the same formulas on the same fp32 inputs, for the bound on the restatement's own rounding).  Nothing here calls the library but to read the
caller's scene through its C view."""
import numpy as np

SHARE = 0.25                                   # KY_PICK_UNIFORM_SHARE
COS_FLOOR = 0.015625                           # KY_PICK_COS_FLOOR
MAX_PROXIES, MAX_CARRIERS, MAX_LIGHTS = 32, 4, 16
SPHERE, PLANAR, POINT, DIRECTION, ENVIRONMENT = 0, 1, 2, 3, 4
BELOW_ONE = np.float32(1.0) - np.float32(2.0 ** -24)
LUM = (np.float32(0.212671), np.float32(0.715160), np.float32(0.072169))   # color_t::luminance, ky.cpp:249
F32 = np.float32


def scene_view(api, scene):
    """the caller's ky_scene as the library reads it"""
    return api._scene_ptr(scene).contents


def _lum64(c):
    e = float(LUM[0]) * float(c[0]) + float(LUM[1]) * float(c[1]) + float(LUM[2]) * float(c[2])
    return min(e, 1e30) if e > 0.0 else 0.0


def _p3(v):
    return np.array([v[0], v[1], v[2]], np.float32)


def shape_area(A, sh):
    """shape_t::area (1141, 1222, 1304, 1401) in fp32, as the host packs DLight::area"""
    pi = F32(3.14159265358979323846)
    cm = lambda u, v: np.sqrt((np.cross(u, v).astype(F32) ** 2).sum(dtype=F32), dtype=F32)
    if sh.kind == A.SHAPE_DISK:
        return pi * F32(sh.radius) * F32(sh.radius)
    if sh.kind == A.SHAPE_TRIANGLE:
        return F32(0.5) * cm(_p3(sh.p[1]) - _p3(sh.p[0]), _p3(sh.p[2]) - _p3(sh.p[0]))
    if sh.kind == A.SHAPE_RECTANGLE:
        return cm(_p3(sh.p[0]) - _p3(sh.p[1]), _p3(sh.p[2]) - _p3(sh.p[1]))
    return F32(4) * pi * (F32(sh.radius) * F32(sh.radius))


def _shape_proxy(A, sh, light, e):
    row = np.zeros(11, np.float64)
    row[0], row[10] = light, e
    if sh.kind in (A.SHAPE_SPHERE, A.SHAPE_DISK):
        row[2:5], row[5] = _p3(sh.p[0]), sh.radius
    else:
        p = [np.array(_p3(sh.p[k]), np.float64) for k in range(3)]
        corners = p if sh.kind == A.SHAPE_TRIANGLE else p + [p[0] + p[2] - p[1]]        # a rectangle samples p1 + (p0 - p1) u + (p2 - p1) v (1310)
        c = sum(corners) / len(corners)
        row[2:5] = c
        row[5] = np.sqrt(max(((q - c) ** 2).sum() for q in corners))
    if sh.kind == A.SHAPE_SPHERE:
        row[1] = SPHERE
    else:
        row[1] = PLANAR
        row[6:9], row[9] = _p3(sh.normal), shape_area(A, sh)
    return row


def host_tables(A, api, scene):
    """-> (proxies [n, 11] fp32 = {light, kind, c[3], r, n[3], A, e}, first [n_lights + 1], power_p [16] fp32): pack_light_pick"""
    s = scene_view(api, scene)
    nl = s.light_count
    carriers = [[] for _ in range(nl)]
    total = nl
    for i in range(nl):
        if s.lights[i].kind != A.LIGHT_AREA:
            continue
        for j in range(s.surface_count):
            if len(carriers[i]) < MAX_CARRIERS and s.surfaces[j].area_light == i and s.surfaces[j].shape != s.lights[i].shape:
                carriers[i].append(s.surfaces[j].shape)
        total += len(carriers[i])
    for i in range(nl - 1, -1, -1):            # a full table: carrier proxies go, from the last light backwards
        if total <= MAX_PROXIES:
            break
        drop = min(len(carriers[i]), total - MAX_PROXIES)
        carriers[i] = carriers[i][:len(carriers[i]) - drop]
        total -= drop
    rows, first, w = [], [], []
    for i in range(nl):
        l = s.lights[i]
        e, R = _lum64(l.color), float(l.world_radius)
        first.append(len(rows))
        row = np.zeros(11, np.float64)
        row[0], row[10] = i, e
        if l.kind == A.LIGHT_AREA:
            row = _shape_proxy(A, s.shapes[l.shape], i, e)
            wi = np.pi * e * float(shape_area(A, s.shapes[l.shape]))
        elif l.kind == A.LIGHT_POINT:
            row[1], row[2:5] = POINT, _p3(l.position)
            wi = 4 * np.pi * e
        elif l.kind == A.LIGHT_DIRECTION:
            row[1], row[2:5] = DIRECTION, -_p3(l.direction)
            wi = np.pi * R * R * e
        else:
            row[1] = ENVIRONMENT
            wi = np.pi * np.pi * R * R * e
        rows.append(row)
        rows += [_shape_proxy(A, s.shapes[k], i, e) for k in carriers[i]]
        w.append(min(wi, 1e30) if wi > 0.0 else 0.0)
    first.append(len(rows))
    W = 0.0
    for wi in w:
        W += wi
    power = np.zeros(MAX_LIGHTS, np.float32)
    for i in range(nl):
        power[i] = SHARE / nl + (1.0 - SHARE) * (w[i] / W) if W > 0.0 else 1.0 / nl
    return np.array(rows, np.float64).reshape(-1, 11).astype(np.float32), np.array(first, np.int64), power


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _materials(A, api, scene, rows16, T):
    """per row: plastic?, kd, ks, Nn, exponent -- the material of the row's surface as the device packs it (pack_material), the two lobe colours as luminances
    times their lobe's probability"""
    s = scene_view(api, scene)
    n = len(rows16)
    plastic, kd, ks, Nn, ex = np.zeros(n, bool), np.ones(n, T), np.zeros(n, T), np.zeros(n, T), np.zeros(n, T)
    per = {}
    for si in range(s.surface_count):
        m = s.materials[s.surfaces[si].material]
        if m.kind != A.MATERIAL_PLASTIC:
            per[si] = None
            continue
        c0 = np.array([F32(m.color0[j]) / F32(m.diffuse_probability) for j in range(3)], np.float32)
        cs = np.array([F32(m.color1[j]) / F32(m.specular_probability) for j in range(3)], np.float32)
        lum = lambda c: T(LUM[0]) * T(c[0]) + T(LUM[1]) * T(c[1]) + T(LUM[2]) * T(c[2])
        ps = T(F32(m.specular_probability))
        per[si] = ((T(1) - ps) * lum(c0), ps * lum(cs), T((F32(m.exponent) + F32(2)) * F32(0.15915494309189535)), T(F32(m.exponent)))
    surf = rows16[:, 9].astype(np.int64)
    for si, v in per.items():
        if v is None:
            continue
        sel = surf == si
        plastic[sel] = True
        kd[sel], ks[sel], Nn[sel], ex[sel] = v
    return plastic, kd, ks, Nn, ex


def spatial_weights(A, api, scene, rows16, T=np.float32, tables=None):
    """-> w [rows, n_lights]: each light's sum over its proxies of clamp(e Om m, 0, 1e30), NaN counting as 0"""
    prox, first, _ = tables if tables is not None else host_tables(A, api, scene)
    nl = len(first) - 1
    rows16 = np.asarray(rows16, np.float32)
    P, N, wo = (rows16[:, k:k + 3].astype(T) for k in (0, 3, 6))
    plastic, kd, ks, Nn, ex = _materials(A, api, scene, rows16, T)
    R = (T(2) * _dot(N, wo))[:, None] * N - wo
    w = np.zeros((len(rows16), nl), T)
    pi, inv_pi = T(F32(np.pi)), T(F32(0.318309886183790671538))
    with np.errstate(all="ignore"):
        for i in range(nl):
            for k in range(first[i], first[i + 1]):
                q = prox[k].astype(T)
                kind, c, r, nq, area, e = int(prox[k][1]), q[2:5], q[5], q[6:9], q[9], q[10]
                if kind == ENVIRONMENT:
                    wk = e * (kd + ks)
                else:
                    sin_t, cos_t, Om = np.zeros(len(P), T), np.ones(len(P), T), np.ones(len(P), T)
                    om = np.broadcast_to(c, P.shape)
                    if kind != DIRECTION:
                        d = c[None, :] - P
                        d2 = np.maximum(_dot(d, d), T(1e-12))
                        inv_d = T(1) / np.sqrt(d2)
                        om = d * inv_d[:, None]
                        if kind == POINT:
                            Om = inv_d * inv_d
                        else:
                            sin_t = np.minimum(T(1), r * inv_d)
                            cos_t = np.sqrt(T(1) - sin_t * sin_t)
                            if kind == SPHERE:
                                Om = ((T(2) * pi) * (sin_t * sin_t)) * (T(1) / (T(1) + cos_t))      # 2 pi (1 - cos_t), without the cancellation
                            else:
                                Om = (area * np.maximum(T(0), -_dot(np.broadcast_to(nq, P.shape), om))) * (T(1) / np.maximum(d2, r * r))
                    cc = np.minimum(np.fmax(_dot(N, om) + sin_t, T(COS_FLOOR)), T(1))           # (fmax: a NaN cosine is the floor, as the device's fmaxf makes it)
                    cos_a = _dot(R, om)
                    x = np.cross(R, om).astype(T)
                    sin_a = np.sqrt(_dot(x, x))                                                     # |R x om|: well conditioned near the mirror direction
                    t = np.where(cos_a >= cos_t, T(1), np.maximum(T(0), cos_a * cos_t + sin_a * sin_t))
                    lobe = Nn * np.power(t, ex)
                    if kind in (SPHERE, PLANAR):
                        lobe = np.minimum(lobe, T(1) / Om)
                    m = np.where(plastic, cc * (kd * inv_pi + ks * lobe), cc)
                    wk = (e * Om) * m
                w[:, i] += np.where(wk > 0, np.minimum(wk, T(1e30)), T(0)).astype(T)
    return w


def spatial_p(w, T=np.float32):
    """every light's probability from the weights: a / n + (1 - a) w / W, W summed in the lights' order; 1 / n where W is 0"""
    n, nl = w.shape
    if nl == 1:
        return np.ones((n, 1), T)
    a, fn = T(SHARE), T(nl)
    W = np.zeros(n, T)
    for i in range(nl):
        W = W + w[:, i]
    with np.errstate(all="ignore"):
        p = a * (T(1) / fn) + (T(1) - a) * (w * (T(1) / W)[:, None])
    return np.where((W > 0)[:, None], p, T(1) / fn).astype(T)


def select_spatial(u, w, T=np.float32):
    """pick_light<spatial>: -> (index, its p, margin).  margin: how far, in units of the pick number, the row's nearest decision was from going the other way --
    the branch (|u - a|), the uniform branch's index, every `t < w` of the weighted branch divided by what the rescalings so far multiplied u' by."""
    u = np.asarray(u, np.float32).astype(T)
    n, nl = w.shape
    if nl == 1:
        return np.zeros(n, np.int64), np.ones(n, T), np.full(n, np.inf)
    a, fn = T(SHARE), T(nl)
    uniform = u < a
    x = (u * (T(1) / a)) * fn
    iu = np.minimum(x.astype(np.int64), nl - 1)
    up = np.minimum((u - a) * (T(1) / (T(1) - a)), T(BELOW_ONE))
    Wp, w_sel, w_uni, sel = np.zeros(n, T), np.zeros(n, T), np.zeros(n, T), np.zeros(n, np.int64)
    amp, margin = np.ones(n, np.float64), np.full(n, np.inf)
    with np.errstate(all="ignore"):
        for i in range(nl):
            wi = w[:, i]
            W = Wp + wi
            t = up * W
            some = wi > 0
            take = some & ((t < wi) | ~(Wp > 0))                           # the first light that weighs anything is taken whatever u' W rounds to
            margin = np.minimum(margin, np.where(some, np.abs(t.astype(np.float64) - wi) / W / amp, np.inf))
            nxt = np.minimum(np.where(take, t, t - wi) * (T(1) / np.where(take, wi, Wp)), T(BELOW_ONE))
            amp = np.where(some, amp * np.where(take, W / wi, W / Wp).astype(np.float64), amp)
            up = np.where(some, nxt, up)
            sel = np.where(take, i, sel)
            w_sel = np.where(take, wi, w_sel)
            w_uni = np.where(iu == i, wi, w_uni)
            Wp = W
        inv_n = T(1) / fn
        p = a * inv_n + (T(1) - a) * (np.where(uniform, w_uni, w_sel) * (T(1) / Wp))
    li = np.where(uniform, iu, sel)
    plain = np.minimum((u * fn).astype(np.int64), nl - 1)                 # all weights zero: 3821 on u itself
    some_w = Wp > 0
    li, p = np.where(some_w, li, plain), np.where(some_w, p, inv_n)
    frac = np.abs(x.astype(np.float64) - np.round(x.astype(np.float64))) / (4.0 * nl)          # the uniform branch's index, back in units of u
    margin = np.where(uniform, frac, margin * (1.0 - SHARE))
    margin = np.minimum(margin, np.abs(u.astype(np.float64) - SHARE))
    plain_m = np.abs((u * fn).astype(np.float64) - np.round((u * fn).astype(np.float64))) / nl
    return li, p.astype(T), np.where(some_w, margin, plain_m)


def select_power(u, power_p, nl):
    """pick_light<power>: the running sum of the 16 probabilities inverted with u, the last light where the sum ends below it -> (index, its p, margin)"""
    u = np.asarray(u, np.float32)
    n = len(u)
    if nl == 1:
        return np.zeros(n, np.int64), np.ones(n, np.float32), np.full(n, np.inf)
    li, p = np.full(n, nl - 1, np.int64), np.full(n, power_p[nl - 1], np.float32)
    open_, cum, margin = np.ones(n, bool), np.float32(0), np.full(n, np.inf)
    for i in range(nl - 1):
        cum = np.float32(cum + power_p[i])
        take = open_ & (u < cum)
        li, p = np.where(take, i, li), np.where(take, power_p[i], p).astype(np.float32)
        open_ &= ~take
        margin = np.minimum(margin, np.abs(u.astype(np.float64) - float(cum)))
    return li, p, margin
