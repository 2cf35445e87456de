"""Not a test: textures (ky_texture) restated in NumPy.  (u, v) of a hit point per shape kind, the (u', v') transform and both look-ups, each
in a float32 path that rounds where section 13 says the device rounds (a fused multiply-add is one rounding of the exact double result) and a float64 path of the same
float32 inputs.  tiled(A, scene, textures) builds the scene in which every textured rectangle is cut along its checker cells or image texels into constant-colour
rectangles: something the unchanged CPU oracle can trace, and therefore the oracle for checker and nearest-image textures on rectangles.
The keyword arguments `swap`, `parity`, `half` and `row0` name defects that tests/test_texture.py shows failing."""
import math

import numpy as np

from helpers import CustomScene

f32, f64 = np.float32, np.float64
CHECKER, IMAGE = 0, 1
BILINEAR, CLAMP = 1, 2
DISK, TRIANGLE, RECTANGLE, SPHERE = 0, 1, 2, 3


def fma(a, b, c, dtype):
    """a b + c rounded once (float32: the product and sum of float32 values are exact enough in double that the one rounding to float32 is the fused result's)"""
    if dtype == f64:
        return np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def mul(a, b, dtype):
    return (np.asarray(a, dtype) * np.asarray(b, dtype)).astype(dtype)


class Shape:
    """kind, p[4][3], normal[3], radius of a ky_shape, float32"""

    def __init__(self, kind, p, normal=(0, 0, 0), radius=0.0):
        self.kind = int(kind)
        self.p = np.zeros((4, 3), f32)
        self.p[:len(p)] = np.asarray(p, f32)
        self.normal = np.asarray(normal, f32)
        self.radius = f32(radius)

    @staticmethod
    def of(s):
        return Shape(s.kind, [[s.p[i][j] for j in range(3)] for i in range(4)], [s.normal[j] for j in range(3)], s.radius)


def frame(n):
    """frame_t(n) for a unit n as the host stores it per surface (float32): t = normalize(n x (|n.x| > 0.99 ? Y : X)), s = t x n"""
    n = np.asarray(n, f32)
    if abs(n[0]) > f32(0.99):
        k = f32(1) / np.sqrt(n[2] * n[2] + n[0] * n[0], dtype=f32)
        t = np.array([-n[2] * k, 0, n[0] * k], f32)
    else:
        k = f32(1) / np.sqrt(n[2] * n[2] + n[1] * n[1], dtype=f32)
        t = np.array([0, n[2] * k, -n[1] * k], f32)
    s = np.array([t[1] * n[2] - t[2] * n[1], t[2] * n[0] - t[0] * n[2], t[0] * n[1] - t[1] * n[0]], f32)
    return s, t


def uv_record(shape):
    """The constants of one surface, computed in double from the shape's floats and rounded once: (kind, o, e1, e2, k0, k1, k2, add) -- kind 1 is the sphere"""
    P = shape.p.astype(f64)
    if shape.kind == SPHERE:
        return 1, shape.p[0], np.zeros(3, f32), np.zeros(3, f32), f32(1.0 / f64(shape.radius)), f32(0), f32(0), f32(0)
    if shape.kind == DISK:
        s, t = frame(shape.normal)
        k = f32(1.0 / (2.0 * f64(shape.radius)))
        return 0, shape.p[0], s, t, k, k, f32(0), f32(0.5)
    e1 = P[1] - P[0]
    e2 = (P[3] if shape.kind == RECTANGLE else P[2]) - P[0]
    g11, g22, g12 = e1 @ e1, e2 @ e2, e1 @ e2
    if shape.kind == RECTANGLE:
        k0, k1, k2 = 1.0 / g11, 1.0 / g22, 0.0
    else:
        det = g11 * g22 - g12 * g12
        k0, k1, k2 = g22 / det, g11 / det, -g12 / det
    return 0, shape.p[0], e1.astype(f32), e2.astype(f32), f32(k0), f32(k1), f32(k2), f32(0)


def uv(shape, p, dtype=f32, swap=False):
    """(u, v) of the points p [n, 3] (float32) of `shape`.  swap: the named defect "u and v swapped on the rectangle"."""
    kind, o, e1, e2, k0, k1, k2, add = uv_record(shape)
    p = np.asarray(p, f32)
    d = (p.astype(dtype) - o.astype(dtype)).astype(dtype)
    if kind == 1:
        nx, ny, nz = mul(d[:, 0], k0, dtype), mul(d[:, 1], k0, dtype), mul(d[:, 2], k0, dtype)
        at = np.arctan2(nz, nx).astype(dtype)
        u = fma(at, dtype(0.15915494309189535), dtype(0.5), dtype)
        v = mul(np.arccos(np.clip(ny, dtype(-1), dtype(1))).astype(dtype), dtype(0.31830988618379067), dtype)
        return u, v
    a = fma(d[:, 2], e1[2], fma(d[:, 1], e1[1], mul(d[:, 0], e1[0], dtype), dtype), dtype)
    b = fma(d[:, 2], e2[2], fma(d[:, 1], e2[1], mul(d[:, 0], e2[0], dtype), dtype), dtype)
    u = (fma(k2, b, mul(k0, a, dtype), dtype) + dtype(add)).astype(dtype)
    v = (fma(k2, a, mul(k1, b, dtype), dtype) + dtype(add)).astype(dtype)
    return (v, u) if (swap and shape.kind == RECTANGLE) else (u, v)


class Tex:
    """What a ky_texture says: kind, material, flags, scale, offset, a, b, texels [h, w, 3] -- all float32"""

    def __init__(self, kind, material, flags=0, scale=(1, 1), offset=(0, 0), a=(0, 0, 0), b=(0, 0, 0), texels=None):
        self.kind, self.material, self.flags = int(kind), int(material), int(flags)
        self.scale, self.offset = np.asarray(scale, f32), np.asarray(offset, f32)
        self.a, self.b = np.asarray(a, f32), np.asarray(b, f32)
        self.texels = None if texels is None else np.ascontiguousarray(texels, f32)

    def to_api(self, api):
        if self.kind == CHECKER:
            return api.texture_checker(self.material, self.a, self.b, self.scale, self.offset)
        return api.texture_image(self.material, self.texels, bool(self.flags & BILINEAR), bool(self.flags & CLAMP), self.scale, self.offset)


def transform(tex, u, v, dtype=f32):
    return fma(tex.scale[0], u, tex.offset[0], dtype), fma(tex.scale[1], v, tex.offset[1], dtype)


def wrap(tex, x, dtype):
    x = np.asarray(x, dtype)
    if tex.flags & CLAMP:
        return np.minimum(np.maximum(x, dtype(0)), dtype(f32(0.99999994)))
    return (x - np.floor(x)).astype(dtype)


def checker(tex, us, vs, parity="sum_of_floors"):
    """colour a where floor(u') + floor(v') is even, b where odd.  parity="floor_of_sum": the named defect, a checker keyed on floor(u' + v')."""
    if parity == "floor_of_sum":
        k = np.floor(np.asarray(us, f64) + np.asarray(vs, f64)).astype(np.int64)
    else:
        k = np.floor(us).astype(np.int64) + np.floor(vs).astype(np.int64)
    return np.where((k & 1)[:, None] == 0, tex.a[None, :], tex.b[None, :]).astype(f32)


def nearest(tex, us, vs, dtype=f32, row0="v0"):
    """texel (min(int(u' W), W - 1), min(int(v' H), H - 1)) of the wrapped coordinates.  row0="v1": the named defect, row 0 at v' = 1."""
    H, W = tex.texels.shape[:2]
    ix = np.minimum(mul(wrap(tex, us, dtype), dtype(W), dtype).astype(np.int64), W - 1)
    iy = np.minimum(mul(wrap(tex, vs, dtype), dtype(H), dtype).astype(np.int64), H - 1)
    if row0 == "v1":
        iy = H - 1 - iy
    return tex.texels[iy, ix]


def wrap_index(tex, i, n):
    return np.clip(i, 0, n - 1) if tex.flags & CLAMP else np.where(i < 0, i + n, np.where(i >= n, i - n, i))


def bilinear(tex, us, vs, dtype=f32, half=True, row0="v0"):
    """pbrt's: the sample position is u' W - 0.5, the four neighbours wrapped or clamped like the coordinate, the lerps a + t (b - a) as fused multiply-adds.
    half=False: the named defect, bilinear without the -0.5."""
    H, W = tex.texels.shape[:2]
    off = dtype(-0.5 if half else 0.0)
    s, t = fma(wrap(tex, us, dtype), dtype(W), off, dtype), fma(wrap(tex, vs, dtype), dtype(H), off, dtype)
    s0, t0 = np.floor(s), np.floor(t)
    ds, dt = (s - s0).astype(dtype), (t - t0).astype(dtype)
    x0, x1 = wrap_index(tex, s0.astype(np.int64), W), wrap_index(tex, s0.astype(np.int64) + 1, W)
    y0, y1 = wrap_index(tex, t0.astype(np.int64), H), wrap_index(tex, t0.astype(np.int64) + 1, H)
    if row0 == "v1":
        y0, y1 = H - 1 - y0, H - 1 - y1
    T = tex.texels.astype(dtype)

    def lerp(w, a, b):
        return fma(w[:, None], (b - a).astype(dtype), a, dtype)
    top, bot = lerp(ds, T[y0, x0], T[y0, x1]), lerp(ds, T[y1, x0], T[y1, x1])
    return lerp(dt, top, bot)


def lookup(tex, us, vs, dtype=f32):
    if tex.kind == CHECKER:
        return checker(tex, us, vs)
    return bilinear(tex, us, vs, dtype) if tex.flags & BILINEAR else nearest(tex, us, vs, dtype)


def probe(shape, tex, p, dtype=f32):
    """(u', v', r, g, b) [n, 5] of the points p of `shape` under `tex`: what kyhip_kat_texture returns"""
    u, v = uv(shape, p, dtype)
    us, vs = transform(tex, u, v, dtype)
    return np.concatenate([np.stack([us, vs], axis=1).astype(dtype), lookup(tex, us, vs, dtype).astype(dtype)], axis=1)


def edge_distance(tex, us, vs):
    """how far (u', v') -- float64 -- lie from the nearest cell or texel edge, in units of u', v'"""
    us, vs = np.asarray(us, f64), np.asarray(vs, f64)
    if tex.kind == CHECKER:
        W = H = 1
    else:
        H, W = tex.texels.shape[:2]
    du = np.abs(us * W - np.round(us * W)) / W
    dv = np.abs(vs * H - np.round(vs * H)) / H
    if tex.kind == IMAGE and tex.flags & CLAMP:   # a clamped coordinate has no edge at 0 or 1, and none beyond
        du = np.where((np.round(us * W) <= 0) | (np.round(us * W) >= W), np.inf, du)
        dv = np.where((np.round(vs * H) <= 0) | (np.round(vs * H) >= H), np.inf, dv)
    return np.minimum(du, dv)


# ---- scenes ----

def copy_scene(A, c, materials_of=None):
    """A CustomScene with the arrays of the ky_scene `c`; materials_of: {surface: ky_material or None} gives each named surface a material of its own -- a copy
    of the one it has, or the given one -- appended behind the scene's.  -> (scene, {surface: its new material index})"""
    shapes = [A.Shape.from_buffer_copy(c.shapes[i]) for i in range(c.shape_count)]
    materials = [A.Material.from_buffer_copy(c.materials[i]) for i in range(c.material_count)]
    lights = [A.Light.from_buffer_copy(c.lights[i]) for i in range(c.light_count)]
    surfaces = [A.Surface.from_buffer_copy(c.surfaces[i]) for i in range(c.surface_count)]
    index = {}
    for s, m in (materials_of or {}).items():
        materials.append(A.Material.from_buffer_copy(m if m is not None else c.materials[surfaces[s].material]))
        surfaces[s].material = index[s] = len(materials) - 1
    return CustomScene(A, A.Camera.from_buffer_copy(c.camera), shapes, materials, lights, surfaces, c.environment_light), index


def cornell_case(A, api, w, h, only_floor=False):
    """The Cornell box under textures -> (scene, [Tex]): a 4 x 4 checker on the floor (surface 3, the plane z = -1.28 the balls stand on; in this scene it is the
    plastic material), a 4 x 4 nearest image on the back wall (surface 4, the matte wall the camera faces) and a checker on the wall x = -1.27 (surface 0), which
    becomes a mirror.  Each of the three surfaces has a material of its own."""
    handle = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)   # (kept until its arrays are copied)
    base = handle.c
    mirror = A.Material.from_buffer_copy(base.materials[base.surfaces[0].material])
    mirror.kind = A.MATERIAL_MIRROR
    scene, idx = copy_scene(A, base, {3: None, 4: None, 0: mirror})
    floor = Tex(CHECKER, idx[3], scale=(4, 4), a=(0.30, 0.28, 0.05), b=(0.04, 0.06, 0.25))
    if only_floor:
        return scene, [floor]
    gen = np.random.default_rng(4)
    image = Tex(IMAGE, idx[4], texels=(0.1 + 0.8 * gen.random((4, 4, 3))).astype(f32))
    wall = Tex(CHECKER, idx[0], scale=(3, 2), offset=(0.25, 0.5), a=(0.9, 0.9, 0.9), b=(0.9, 0.3, 0.2))
    return scene, [floor, image, wall]


def veach_case(A, api, w, h):
    """create_mis_scene under textures -> (scene, [Tex]): a checker on one plank (surface 2, plastic) and on the floor (surface 0, matte), each on a material of
    its own (the planks share one, the floor shares the wall's)."""
    handle = api.mis_scene(w, h)
    base = handle.c
    scene, idx = copy_scene(A, base, {2: None, 0: None})
    plank = Tex(CHECKER, idx[2], scale=(2, 8), a=(0.07, 0.09, 0.13), b=(0.20, 0.05, 0.03))
    floor = Tex(CHECKER, idx[0], scale=(10, 10), offset=(0.5, 0.25), a=(0.4, 0.4, 0.4), b=(0.1, 0.2, 0.3))
    return scene, [plank, floor]


def cuts(tex, axis, subdivide=1):
    """the values of u (axis 0) or v (axis 1) in (0, 1) at which the texture's cell or texel changes along a surface's edge, ascending, in double; subdivide: that
    many tiles per cell"""
    s, o = f64(tex.scale[axis]), f64(tex.offset[axis])
    n = 1 if tex.kind == CHECKER else tex.texels.shape[1 - axis]
    lo, hi = sorted((o, s + o))   # u' over u in [0, 1]
    if tex.kind == IMAGE and tex.flags & CLAMP:
        lo, hi = max(lo, 0.0), min(hi, 1.0)
    out = []
    k = math.floor(lo * n * subdivide) - 1
    while k / (n * subdivide) <= hi:
        u = (k / (n * subdivide) - o) / s
        if 1e-9 < u < 1 - 1e-9:
            out.append(u)
        k += 1
    return sorted(out)


def tiled(A, c, textures, subdivide=1):
    """The ky_scene `c` with every textured rectangle cut along its checker cells or image texels (subdivide x subdivide tiles per cell): the tiles stand at the
    original surface's place in the surface list, in v-major order; each takes a copy of the surface's material with color0 = the texture's value at the tile's
    centre (one material per colour), so a plastic tile keeps its diffuse_probability / specular_probability.  Only checker and nearest textures have constant
    tiles; only parallelograms are cut.  New shapes and materials are appended, so every index the lights hold stays valid."""
    shapes = [A.Shape.from_buffer_copy(c.shapes[i]) for i in range(c.shape_count)]
    materials = [A.Material.from_buffer_copy(c.materials[i]) for i in range(c.material_count)]
    lights = [A.Light.from_buffer_copy(c.lights[i]) for i in range(c.light_count)]
    by_material = {t.material: t for t in textures}
    surfaces = []
    colour_material = {}
    for i in range(c.surface_count):
        sf = c.surfaces[i]
        tex = by_material.get(sf.material)
        sh = Shape.of(c.shapes[sf.shape])
        if tex is None or sh.kind != RECTANGLE:
            surfaces.append(A.Surface.from_buffer_copy(sf))
            continue
        assert tex.kind == CHECKER or not (tex.flags & BILINEAR), "a bilinear texture has no constant tiles"
        P = sh.p.astype(f64)
        e1, e3 = P[1] - P[0], P[3] - P[0]
        assert np.abs(P[0] + e1 + e3 - P[2]).max() < 1e-6, "only parallelograms are cut"
        us, vs = [0.0] + cuts(tex, 0, subdivide) + [1.0], [0.0] + cuts(tex, 1, subdivide) + [1.0]
        for b in range(len(vs) - 1):
            for a in range(len(us) - 1):
                uc, vc = 0.5 * (us[a] + us[a + 1]), 0.5 * (vs[b] + vs[b + 1])
                tus, tvs = transform(tex, np.array([uc]), np.array([vc]), f64)
                col = tuple(float(x) for x in lookup(tex, tus, tvs, f64)[0])
                key = (sf.material, col)
                if key not in colour_material:
                    m = A.Material.from_buffer_copy(c.materials[sf.material])
                    for j in range(3):
                        m.color0[j] = col[j]
                    materials.append(m)
                    colour_material[key] = len(materials) - 1
                s = A.Shape.from_buffer_copy(c.shapes[sf.shape])
                corners = (P[0] + us[a] * e1 + vs[b] * e3, P[0] + us[a + 1] * e1 + vs[b] * e3, P[0] + us[a + 1] * e1 + vs[b + 1] * e3, P[0] + us[a] * e1 + vs[b + 1] * e3)
                for k, q in enumerate(corners):
                    for j in range(3):
                        s.p[k][j] = float(q[j])
                shapes.append(s)
                surfaces.append(A.Surface(len(shapes) - 1, colour_material[key], sf.area_light))
    return CustomScene(A, A.Camera.from_buffer_copy(c.camera), shapes, materials, lights, surfaces, c.environment_light)
