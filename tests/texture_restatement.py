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
        # tex_uv's u is d . e1 / |e1|^2: on a sheared parallelogram that is not the coordinate the cuts below run along
        assert abs(e1 @ e3) <= 1e-6 * np.sqrt((e1 @ e1) * (e3 @ e3)), "only parallelograms whose edges are orthogonal are cut"
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


# ---- the texel layout of a set (texture_pack), and the defects it can have ----

def texels_of(k, w, h):
    """Image k, [h, w, 3]: texel (x, y) is ((x + 1) / 8, (y + 1) / 8, (k + 1) / 16), exact in float32 -- a nearest look-up's colour names the texel it read"""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return np.stack([(x + 1) / 8.0, (y + 1) / 8.0, np.full((h, w), (k + 1) / 16.0)], axis=2).astype(f32)


def pack(textures):
    """texture_pack's texel array restated: every texture's texels one behind the other in set order, an image row by row from row 0, a checker as the 2 x 1
    image {a, b} -> (flat [n, 3] float32, [first texel of each texture])"""
    flat, first = [], []
    for t in textures:
        first.append(sum(len(f) for f in flat))
        flat.append(np.stack([t.a, t.b]) if t.kind == CHECKER else t.texels.reshape(-1, 3))
    return np.concatenate(flat).astype(f32), first


def nearest_packed(textures, i, us, vs, dtype=f32, defect=None):
    """nearest() of image i of a set through the packed array: texel first + iy W + ix.  The named defects: "transposed" reads first + ix H + iy, "stride_h"
    first + iy H + ix, "no_first" iy W + ix."""
    tex = textures[i]
    flat, first = pack(textures)
    H, W = tex.texels.shape[:2]
    ix = np.minimum(mul(wrap(tex, us, dtype), dtype(W), dtype).astype(np.int64), W - 1)
    iy = np.minimum(mul(wrap(tex, vs, dtype), dtype(H), dtype).astype(np.int64), H - 1)
    idx = {None: first[i] + iy * W + ix, "transposed": first[i] + ix * H + iy, "stride_h": first[i] + iy * H + ix, "no_first": iy * W + ix}[defect]
    return flat[idx]


# ---- a scene that textures every shape kind ----

SKEW = [(0.0, 0.0, 0.0), (3.0, 0.0, 0.0), (4.0, 2.5, 0.0), (-0.5, 2.0, 0.0)]   # the probe's quad that is no parallelogram


def interleaved(A, base, new_shapes, new_materials, new_surfaces, at):
    """The ky_scene `base` with shapes and materials appended and new_surfaces[k] = (shape offset, material) put at place at[k] of the caller's surface list"""
    scene, _ = copy_scene(A, base)
    shapes, mats, lights, surfaces = scene._keep
    n_shapes = len(shapes)
    shapes += list(new_shapes)
    mats += list(new_materials)
    for (sh, m), where in sorted(zip(new_surfaces, at), key=lambda e: e[1]):
        surfaces.insert(where, A.Surface(n_shapes + sh, m, -1))
    return CustomScene(A, A.Camera.from_buffer_copy(base.camera), shapes, mats, lights, surfaces, base.environment_light)


def _matte(A, c):
    from helpers import make_material
    return make_material(A, A.MATERIAL_MATTE, c)


def shapes_case(A, api, w, h, shipped=False):
    """The Cornell box with a texture on every shape kind -> (scene, [Tex], {name: caller's surface index}).  Added: a free triangle, a tilted disk, the probe's
    skew quad (a quarter its size, facing the camera) and a second ball that SHARES the triangle's material; the small mirror ball turns matte.  The caller's list
    interleaves the kinds -- rectangle, triangle, rectangle, disk, rectangle, sphere, rectangle, quad, rectangle, sphere ... -- so a sort by kind permutes it.
    Textures, all on matte materials: a 3 x 5 nearest image on the back wall (a face of the room's box), a 7 x 2 nearest clamped image with negative scale[1] on the
    ball, one checker with non-integer scale and an offset on the triangle's material (triangle and second ball), a 5 x 3 bilinear repeating image on the disk, a
    second checker on the quad.  The bilinear image sits on a planar shape on purpose: its colour is continuous in the hit point, the expected colour is taken at the
    ORACLE's hit point, and a sphere's hit distance -b - sqrt(b^2 - c) cancels (b^2 is about 17 here), so the two sides' float32 hit points on a ball lie several 1e-6
    apart whichever is nearer the truth -- more than the bilinear tolerance; a planar hit distance is one quotient.  (Bilinear look-ups on a sphere are held to the
    restatement at GIVEN points by the probe tests.)  shipped: without triangle, disk and quad, so that the launch keeps the row of the shipped shapes -- whose
    surfaces are balls and faces of boxes, so this set has no bilinear image; the second ball keeps its checker and the second checker goes to the wall x = -1.27."""
    from helpers import make_shape
    handle = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    base = handle.c
    assert base.surface_count == 12 and base.shapes[base.surfaces[5].shape].kind == SPHERE and base.materials[base.surfaces[5].material].kind == A.MATERIAL_MIRROR
    m0 = base.material_count
    mats = [_matte(A, (0.2, 0.3, 0.7)), _matte(A, (0.7, 0.6, 0.5)), _matte(A, (0.6, 0.7, 0.3)), _matte(A, (0.5, 0.5, 0.6)), _matte(A, (0.7, 0.4, 0.4))]
    wall_m, ball_m, tri_m, disk_m, quad_m = range(m0, m0 + 5)
    ball2 = make_shape(A, A.SHAPE_SPHERE, [(0.05, -0.3, 0.7)], radius=0.3)
    if shipped:
        scene = interleaved(A, base, [ball2], mats, [(0, tri_m)], [1])
        names = {"left": 0, "ball2": 1, "wall": 5, "ball": 6}
    else:
        tri = make_shape(A, A.SHAPE_TRIANGLE, [(-1.0, -0.6, 0.1), (-0.6, -0.5, 1.0), (-0.1, -0.9, 0.3)])
        disk = make_shape(A, A.SHAPE_DISK, [(0.75, -0.5, 0.45)], normal=(-0.36, 0.8, 0.48), radius=0.4)
        quad = make_shape(A, A.SHAPE_RECTANGLE, [(0.45 - 0.25 * x, -0.9, -0.35 + 0.25 * y) for x, y, _ in SKEW])
        # base: left 0, right 1, top 2, floor 3, wall 4, ball 5, glass ball 6, lamp 7 .. 11
        scene = interleaved(A, base, [tri, disk, ball2, quad], mats, [(0, tri_m), (1, disk_m), (2, tri_m), (3, quad_m)], [1, 3, 5, 7])
        names = {"left": 0, "tri": 1, "disk": 3, "ball2": 5, "quad": 7, "wall": 8, "ball": 9}
    c = scene.scene
    c.surfaces[names["wall"]].material, c.surfaces[names["ball"]].material = wall_m, ball_m
    if shipped:
        c.surfaces[names["left"]].material = disk_m
    for name, kind in (("wall", RECTANGLE), ("ball", SPHERE), ("ball2", SPHERE), ("tri", TRIANGLE), ("disk", DISK), ("quad", RECTANGLE), ("left", RECTANGLE)):
        assert name not in names or c.shapes[c.surfaces[names[name]].shape].kind == kind, name
    textures = [Tex(IMAGE, ball_m, CLAMP, scale=(1.5, -1.5), offset=(-0.2, 1.2), texels=texels_of(2, 7, 2)),
                Tex(CHECKER, tri_m, scale=(3.5, 2.5), offset=(0.3, -0.2), a=(0.9, 0.8, 0.1), b=(0.1, 0.2, 0.7)),
                Tex(IMAGE, wall_m, 0, scale=(2.3, 1.7), offset=(0.15, 0.4), texels=texels_of(0, 3, 5)),
                Tex(CHECKER, quad_m if not shipped else disk_m, scale=(2.5, 3.5), offset=(0.25, 0.6), a=(0.8, 0.3, 0.2), b=(0.2, 0.7, 0.6))]
    if not shipped:
        textures.append(Tex(IMAGE, disk_m, BILINEAR, scale=(2.0, 1.0), offset=(0.1, 0.05), texels=texels_of(1, 5, 3)))
    scene._keep_handle = handle
    return scene, textures, names


def shapes_case_shipped(A, api, w, h):
    return shapes_case(A, api, w, h, shipped=True)


def shapes_case_large(A, api, w, h):
    """tests/test_stratified_gpu.py's large_scene -- the Cornell box and 65 small balls -- with a checker on the balls' matte material: more than 64 surfaces, and
    33 uv records behind one texture"""
    import test_stratified_gpu as T
    scene = T.large_scene(A, api, w, h)
    c = scene.scene
    m = c.surfaces[12].material
    balls = [i for i in range(c.surface_count) if c.surfaces[i].material == m]
    assert c.surface_count == 77 and len(balls) == 33 and c.materials[m].kind == A.MATERIAL_MATTE and all(c.shapes[c.surfaces[i].shape].kind == SPHERE for i in balls)
    return scene, [Tex(CHECKER, m, scale=(4.0, 2.0), offset=(0.3, 0.1), a=(0.9, 0.8, 0.1), b=(0.1, 0.2, 0.7))], {"balls": balls}


def flat_textures(textures):
    """the control set: every texture replaced by a checker with a == b, a colour of its own each (a silhouette between two textured surfaces shows)"""
    return [Tex(CHECKER, t.material, scale=(3.0, 2.0), offset=(0.5, 0.25), a=(0.25 + 0.125 * i, 0.875 - 0.125 * i, 0.5), b=(0.25 + 0.125 * i, 0.875 - 0.125 * i, 0.5))
            for i, t in enumerate(textures)]


class FirstHits:
    """what expected_samples returns"""


def expected_samples(O, A, scene, textures, params, stride=64, record_of=None, with_k=True):
    """Every sample [h, w, N] of the frame `params` as the oracle and the restatement give it under INTEGRATOR_BASECOLOR:
      surface, position  the oracle's first hit of the tape's camera ray (kyo_kat_camera, kyo_kat_scene_intersect: what kyo_trace_li's first row holds), caller's index;
      k                  kyo_li_tape under basecolor on the scene with every textured material's color0 = (1, 1, 1);
      expected           k x probe(shape, texture, position, float64)'s colour on a textured surface, k elsewhere (float64);
      textured, bilinear, clean (>= 1e-4 from a cell or texel edge and, on a sphere, from the seam u = 0 = 1; every untextured sample is clean), e_ref (the float32
      restatement's largest distance from the float64 one over the bilinear samples).
    record_of {surface: surface}: the named plumbing defects -- a surface's (u, v) taken from ANOTHER surface's shape.  with_k=False: k = 1 (no oracle replay)."""
    import filter_restatement as F
    c = scene.scene
    w, h, n = params.width, params.height, params.samples_per_pixel
    tapes = np.stack([np.stack([F.tape(params.seed, y * w + x, n, stride, params.sampler, None) for x in range(w)]) for y in range(h)]).astype(f32)
    px = (np.arange(w, dtype=f32)[None, :, None] + tapes[..., 0]).astype(f32)
    py = (np.arange(h, dtype=f32)[:, None, None] + tapes[..., 1]).astype(f32)
    rays = O.kat_camera(c.camera, np.stack([px, py], axis=-1).reshape(-1, 2))
    hit = O.kat_scene_intersect(scene, np.concatenate([rays, np.full((len(rays), 1), np.inf, f32)], axis=1))
    out = FirstHits()
    out.tapes = tapes
    out.surface = np.where(hit[:, 0] > 0, hit[:, 8].astype(np.int64), -1)
    out.position = hit[:, 2:5].copy()
    by_material = {t.material: t for t in textures}
    white = copy_scene(A, c)[0]
    for m in by_material:
        assert c.materials[m].kind == A.MATERIAL_MATTE   # (basecolor is linear in a matte colour)
        for j in range(3):
            white.materials[m].color0[j] = 1.0
    bp = A.RenderParams.from_buffer_copy(params)
    bp.integrator = A.INTEGRATOR_BASECOLOR
    k = np.ones((h, w, n, 3), f32)
    for y in range(h if with_k else 0):
        for x in range(w):
            k[y, x] = O.li_tape(white, bp, x, y, tapes[y, x])[0]
    out.k = k.reshape(-1, 3)
    colour = np.ones((len(hit), 3), f64)
    out.textured, out.bilinear, out.clean = np.zeros(len(hit), bool), np.zeros(len(hit), bool), np.ones(len(hit), bool)
    out.e_ref = 0.0
    for s in range(c.surface_count):
        tex = by_material.get(c.surfaces[s].material)
        rows = out.surface == s
        if tex is None or not rows.any():
            continue
        shape = Shape.of(c.shapes[c.surfaces[(record_of or {}).get(s, s)].shape])
        r64 = probe(shape, tex, out.position[rows], f64)
        colour[rows] = r64[:, 2:]
        out.textured[rows] = True
        clean = edge_distance(tex, r64[:, 0], r64[:, 1]) >= 1e-4
        if shape.kind == SPHERE:
            u = uv(shape, out.position[rows], f64)[0]
            clean &= np.minimum(u, 1 - u) >= 1e-4
        out.clean[rows] = clean
        if tex.kind == IMAGE and tex.flags & BILINEAR:
            out.bilinear[rows] = True
            out.e_ref = max(out.e_ref, float(np.abs(probe(shape, tex, out.position[rows], f32)[:, 2:].astype(f64) - r64[:, 2:]).max()))
    out.expected = out.k.astype(f64) * colour
    out.shape = (h, w, n)
    for a in (out.surface, out.position, out.k, out.expected, out.textured, out.bilinear, out.clean):
        a.setflags(write=False)
    return out


# ---- edge coordinates ----

EDGE_RECT = [(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 0.0, 4.0), (0.0, 0.0, 4.0)]   # |e1|^2 = 4, |e2|^2 = 16: (u, v) of (2 u, 0, 4 v) is exact


def edge_points(uvs):
    uvs = np.asarray(uvs, f32)
    return np.stack([f32(2) * uvs[:, 0], np.zeros(len(uvs), f32), f32(4) * uvs[:, 1]], axis=1).astype(f32)


def edge_cases(material=0):
    """name -> (Tex, (u, v) [n, 2] float32 of points of EDGE_RECT): coordinates u' that sit exactly on integers and on k / W, at -2^-30 (where the repeat wrap rounds
    to 1 and the index is capped), beyond +-1000, beyond [0, 1] under clamp, and at the rectangle's corners.  |u'| < 2^24 throughout.  tests/test_texture.py pins
    the float32 restatement at these points to hand-written texel indices."""
    below = lambda x: np.nextafter(f32(x), f32(0))
    corners = [(0, 0), (1, 0), (1, 1), (0, 1)]
    img, img5 = texels_of(0, 4, 2), texels_of(1, 5, 3)
    a, b = (0.9, 0.8, 0.1), (0.1, 0.2, 0.7)
    return {
        "on k / W": (Tex(IMAGE, material, texels=img), [(0, 0.25), (0.25, 0.25), (0.5, 0.25), (0.75, 0.25), (1, 0.25), (0.5, 0.5), (below(0.5), below(0.5))] + corners),
        "-2^-30": (Tex(IMAGE, material, offset=(-2.0 ** -30, 0), texels=img), [(0, 0.25), (0.25, 0.25), (0.5, 0.75)]),
        "beyond 1000": (Tex(IMAGE, material, scale=(4096, 1), offset=(-2048, 0), texels=img), [(0, 0.25), (1, 0.25), (0.5 + 2.0 ** -14, 0.25), (2.0 ** -13, 0.25),
                                                                                              (1 - 3 * 2.0 ** -14, 0.75)]),
        "clamped": (Tex(IMAGE, material, CLAMP, scale=(3, -2), offset=(-1, 1.5), texels=img), [(0, 0), (1, 1), (0.5, 0.5), (0.75, 0.625)] + corners),
        "on k / 5": (Tex(IMAGE, material, texels=img5), [(f32(0.2), f32(1 / 3)), (f32(0.4), f32(2 / 3)), (f32(0.6), f32(1 / 3)), (f32(0.8), below(1 / 3)), (below(0.2), 0.5)]),
        "checker on integers": (Tex(CHECKER, material, scale=(4, 2), a=a, b=b), [(0, 0.25), (0.25, 0.25), (0.5, 0.25), (0.75, 0.25), (1, 0.25), (0.25, 0.5)] + corners),
        "checker beyond 1000": (Tex(CHECKER, material, scale=(4096, 1), offset=(-2048, 0), a=a, b=b), [(0, 0.25), (2.0 ** -13, 0.25), (2.0 ** -12, 0.25), (1, 0.25), (1, 1)]),
        "checker -2^-30": (Tex(CHECKER, material, offset=(-2.0 ** -30, 0), a=a, b=b), [(0, 0.25), (0.5, 0.25), (0, 1)]),
    }
