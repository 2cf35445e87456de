"""Python plumbing over the C ABI (include/kyhip.h) and the C++ host layer (ky_amd/host/ky.hpp).

Nothing here computes radiance: every function forwards to libkyhip.so (HIP kernels) or to the C++ host
classes.  numpy is used for host buffers only.
"""
import ctypes as C

import numpy as np

from . import _abi as A


class KyError(RuntimeError):
    pass


def _check(rc, lib=None):
    if rc != A.KY_OK:
        lib = lib or A.load_kyhip()
        raise KyError(f"kyhip error {rc}: {lib.kyhip_last_error().decode()}")


def _fptr(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


class SceneHandle:
    """A scene built by the C++ host layer (scene_t::create_*_scene) plus its flat C-ABI view."""

    def __init__(self, ptr):
        if not ptr:
            raise KyError("scene creation failed: " + A.load_kyhost().kyhost_last_error().decode())
        self._ptr = C.c_void_p(ptr)
        self._host = A.load_kyhost()
        self.flat = self._host.kyhost_scene_flatten(self._ptr)
        if not self.flat:
            raise KyError("scene flatten failed: " + self._host.kyhost_last_error().decode())

    def __del__(self):
        try:
            if self._ptr:
                self._host.kyhost_scene_destroy(self._ptr)
                self._ptr = None
        except Exception:
            pass

    @property
    def c(self):
        return self.flat.contents

    def _retextured(self, rc):
        if rc != 0:
            raise KyError("texture: " + self._host.kyhost_last_error().decode())
        self.flat = self._host.kyhost_scene_flatten(self._ptr)   # (the material's struct colour is now the texture's base colour)

    def texture_checker(self, material, a, b, scale=(1, 1), offset=(0, 0)):
        """Material `material` rebuilt from a checker_texture_t (ky.hpp: the texture overloads of matte_material_t, mirror_material_t, plastic_material_t): the host
        mirror's render entries then render the scene textured, and textures() is the set they hand to the C ABI."""
        f = lambda v: np.ascontiguousarray(v, np.float32)
        a, b, scale, offset = f(a), f(b), f(scale), f(offset)
        self._retextured(self._host.kyhost_scene_texture_checker(self._ptr, int(material), _fptr(a), _fptr(b), _fptr(scale), _fptr(offset)))

    def texture_image(self, material, array, bilinear=False, clamp=False, scale=(1, 1), offset=(0, 0)):
        """Material `material` rebuilt from an image_texture_t of array[h, w, 3] (copied)."""
        texels = np.ascontiguousarray(array, np.float32)
        scale, offset = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(offset, np.float32)
        self._retextured(self._host.kyhost_scene_texture_image(self._ptr, int(material), int(texels.shape[1]), int(texels.shape[0]), _fptr(texels), int(bilinear), int(clamp),
                                                               _fptr(scale), _fptr(offset)))

    def textures(self):
        """scene_t::flatten_textures(): the ky_texture set of the scene's textured materials (valid while the scene lives and is not retextured)."""
        n = self._host.kyhost_scene_textures(self._ptr, None, 0)
        if n < 0:
            raise KyError("textures: " + self._host.kyhost_last_error().decode())
        arr = (A.Texture * max(n, 1))()
        self._host.kyhost_scene_textures(self._ptr, arr, n)
        return [arr[i] for i in range(n)]

    @property
    def ptr(self):
        return self._ptr


def cornell_box_scene(flags, width, height):
    """scene_t::create_cornell_box_scene(flags, {width, height}) -- ky.cpp:3240."""
    return SceneHandle(A.load_kyhost().kyhost_scene_create_cornell_box(int(flags), float(width), float(height)))


def mis_scene(width, height):
    """scene_t::create_mis_scene({width, height}) -- ky.cpp:3434."""
    return SceneHandle(A.load_kyhost().kyhost_scene_create_mis(float(width), float(height)))


def make_params(width, height, spp, integrator=A.INTEGRATOR_PATH_TRACING_ITERATION, max_path_depth=5,
                direct_sample=A.DIRECT_BOTH_MIS, sampler=A.SAMPLER_RANDOM, seed=1234, tile_w=16, tile_h=16,
                tile_first=0, tile_step=1):
    return A.RenderParams(integrator, max_path_depth, direct_sample, spp, sampler, seed, width, height, tile_w, tile_h,
                          tile_first, tile_step)


def _scene_ptr(scene):
    """A SceneHandle, any object with a `.flat` POINTER(Scene) (e.g. a scene assembled from ctypes structs), or the pointer itself."""
    return scene.flat if hasattr(scene, "flat") else scene


def pixel_filter(kind, radius=None, param=None):
    """A ky_pixel_filter (_abi.PixelFilter): kyhip_filter_defaults(kind) -- tent radius 2, Gaussian radius 1.5 sigma 0.5, Blackman-Harris radius 2 -- with `radius`
    and `param` (the Gaussian's sigma) replaced where given, then kyhip_filter_check, which raises KyError for what it refuses."""
    lib = A.load_kyhip()
    f = A.PixelFilter()
    _check(lib.kyhip_filter_defaults(int(kind), C.byref(f)), lib)
    if radius is not None:
        f.radius = float(radius)
    if param is not None:
        f.param = float(param)
    _check(lib.kyhip_filter_check(C.byref(f)), lib)
    return f


def filter_table(filter):
    """kyhip_filter_table (host only): the FILTER_TABLE + 1 float32 of the filter's inverse CDF, entry i = F^-1(i / FILTER_TABLE) in pixels from the pixel's centre."""
    lib = A.load_kyhip()
    out = np.zeros(A.FILTER_TABLE + 1, np.float32)
    _check(lib.kyhip_filter_table(C.byref(filter), _fptr(out), out.size), lib)
    return out


def kat_filter(filter, u, device=0):
    """kyhip_kat_filter: the filter's warp of each u in [0, 1) -- the camera sample's offset from its pixel's corner along one axis."""
    lib = A.load_kyhip()
    u = np.ascontiguousarray(u, np.float32).ravel()
    out = np.zeros(u.size, np.float32)
    _check(lib.kyhip_kat_filter(device, C.byref(filter), _fptr(u), int(u.size), _fptr(out)))
    return out


def lens(radius, focus_distance=0.0):
    """A ky_lens (_abi.Lens): the aperture radius and the depth of the focus plane along the camera's front, both in world units, through kyhip_lens_check, which
    raises KyError for what it refuses.  radius 0 is the pinhole camera; focus_distance(scene, x, y) finds the depth of what a pixel shows."""
    lib = A.load_kyhip()
    l = A.Lens(float(radius), float(focus_distance), (0, 0))
    _check(lib.kyhip_lens_check(C.byref(l)), lib)
    return l


def kat_lens(u2, device=0):
    """kyhip_kat_lens: the lens's disk map -- Shirley's concentric map -- of each pair u2[i] in [0, 1)^2 -> float32 [n, 2], points of the unit disk."""
    lib = A.load_kyhip()
    u2 = np.ascontiguousarray(u2, np.float32).reshape(-1, 2)
    out = np.zeros(u2.shape, np.float32)
    _check(lib.kyhip_kat_lens(device, _fptr(u2), int(u2.shape[0]), _fptr(out)))
    return out


def focus_distance(scene, x, y, device=0):
    """The depth along the camera's front of what the pinhole ray through the centre of pixel (x, y) hits (kyhip_kat_camera, kyhip_kat_scene_intersect): the
    focus_distance of a lens focused on it.  Raises KyError if the ray hits nothing."""
    cam = _scene_ptr(scene).contents.camera
    ray = kat_camera(cam, np.array([[x + 0.5, y + 0.5]], np.float32), device=device)[0]
    hit = kat_scene_intersect(scene, np.array([list(ray) + [np.inf]], np.float32), device=device)[0]
    if hit[0] == 0:
        raise KyError("focus_distance: the camera ray through pixel (%d, %d) hits nothing" % (x, y))
    front = np.array(list(cam.front), np.float64)
    return float(np.dot(hit[2:5].astype(np.float64) - np.array(list(cam.position), np.float64), front) / np.linalg.norm(front))


def texture_checker(material, a, b, scale=(1, 1), offset=(0, 0)):
    """A checker ky_texture (_abi.Texture) on ky_scene material `material`, whose color0 it replaces: colour a where floor(u') + floor(v') is even, b where it is
    odd, (u', v') = scale * (u, v) + offset.  A texture is checked against its scene where it is used (texture_check)."""
    t = A.Texture(A.TEXTURE_CHECKER, int(material), 0, 0, tuple(float(v) for v in scale), tuple(float(v) for v in offset), tuple(float(v) for v in a),
                  tuple(float(v) for v in b), 0, 0, None)
    return t


def texture_image(material, array, bilinear=False, clamp=False, scale=(1, 1), offset=(0, 0)):
    """An image ky_texture on material `material`: array[h, w, 3], row 0 at v' = 0; nearest or bilinear (pbrt's), repeating or clamped.  The texture keeps the
    float32 copy of the array it points to alive."""
    texels = np.ascontiguousarray(array, np.float32)
    if texels.ndim != 3 or texels.shape[2] != 3:
        raise ValueError("texture_image: array[h, w, 3]")
    t = A.Texture(A.TEXTURE_IMAGE, int(material), (A.TEXTURE_BILINEAR if bilinear else 0) | (A.TEXTURE_CLAMP if clamp else 0), 0, tuple(float(v) for v in scale),
                  tuple(float(v) for v in offset), (0, 0, 0), (0, 0, 0), int(texels.shape[1]), int(texels.shape[0]), texels.ctypes.data_as(C.POINTER(C.c_float)))
    t._texels = texels
    return t


def _texture_array(textures):
    """(a contiguous ky_texture array or None, n) of a sequence of textures; the sequence keeps the texels alive"""
    textures = list(textures) if textures is not None else []
    if not textures:
        return None, 0
    arr = (A.Texture * len(textures))()
    for i, t in enumerate(textures):
        C.memmove(C.byref(arr, i * C.sizeof(A.Texture)), C.byref(t), C.sizeof(A.Texture))
    return arr, len(textures)


def texture_check(scene, textures):
    """kyhip_texture_check (host only): raises KyError for a set that `scene` refuses -- a glass or out-of-range material, two textures on one material, a negative or
    non-finite colour or texel, a scale of 0, an image without texels, or a set beyond the limits."""
    lib = A.load_kyhip()
    arr, n = _texture_array(textures)
    _check(lib.kyhip_texture_check(_scene_ptr(scene), arr, n), lib)


def kat_texture(scene, textures, surface, points, device=0):
    """kyhip_kat_texture: (u', v', r, g, b) float32 [n, 5] of world points [n, 3] on surface `surface`, through the device functions the textured kernels call."""
    lib = A.load_kyhip()
    arr, n = _texture_array(textures)
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    out = np.zeros((points.shape[0], 5), np.float32)
    _check(lib.kyhip_kat_texture(device, _scene_ptr(scene), arr, n, int(surface), _fptr(points), int(points.shape[0]), _fptr(out)), lib)
    return out


def render(scene, params, film=None, device=0, row_stride_px=None, origin_px=(0, 0), lighting=None, filter=None, lens=None, textures=None):
    """kyhip_render: integrator_t::render(scene, sampler, film) on the GPU; returns the (accumulated) host film.
    lighting: a mask of LIGHTING_EMIT / _DIRECT / _INDIRECT -- kyhip_render_lighting, only those light classes are added.
    filter: a pixel_filter(...) -- kyhip_render_filtered, the camera samples drawn from the filter's density (not together with lighting).
    lens: a lens(...) -- kyhip_render_lens, the camera rays leave from a disk and meet on the focus plane (with or without filter, not together with lighting)."""
    lib = A.load_kyhip()
    if (filter is not None or lens is not None or textures) and lighting is not None:
        raise ValueError("a render under a pixel filter, a lens or textures has no masked form: filter= / lens= / textures= or lighting=, not both")
    if film is None:
        film = np.zeros((params.height, params.width, 3), np.float32)
    stride = film.shape[1] if row_stride_px is None else row_stride_px
    base = film.ctypes.data + (origin_px[1] * stride + origin_px[0]) * 12
    if textures:   # kyhip_render_textured: the materials' colours from a texture set (texture_checker, texture_image), with or without filter and lens
        arr, n = _texture_array(textures)
        _check(lib.kyhip_render_textured(device, _scene_ptr(scene), arr, n, C.byref(params), C.byref(filter) if filter is not None else None,
                                         C.byref(lens) if lens is not None else None, C.c_void_p(base), stride))
    elif lens is not None:
        _check(lib.kyhip_render_lens(device, _scene_ptr(scene), C.byref(params), C.byref(filter) if filter is not None else None, C.byref(lens), C.c_void_p(base), stride))
    elif filter is not None:
        _check(lib.kyhip_render_filtered(device, _scene_ptr(scene), C.byref(params), C.byref(filter), C.c_void_p(base), stride))
    elif lighting is None:
        _check(lib.kyhip_render(device, _scene_ptr(scene), C.byref(params), C.c_void_p(base), stride))
    else:
        _check(lib.kyhip_render_lighting(device, _scene_ptr(scene), C.byref(params), int(lighting), C.c_void_p(base), stride))
    return film


def lighting_plan(params, lighting):
    """kyhip_lighting_plan (host only): (effective_depth, dropped) of render(..., lighting=lighting); effective_depth -1: nothing is launched."""
    lib = A.load_kyhip()
    depth, dropped = C.c_int(0), C.c_int(0)
    _check(lib.kyhip_lighting_plan(C.byref(params), int(lighting), C.byref(depth), C.byref(dropped)), lib)
    return depth.value, dropped.value


def pass_boundaries(spp):
    """kyhip_pass_boundaries (host only): the sample counts at which a pass of an spp-sample frame can end, ascending; the last is spp."""
    lib = A.load_kyhip()
    n = lib.kyhip_pass_boundaries(int(spp), None, 0)
    if n < 0:
        _check(n, lib)
    out = (C.c_int * n)()
    lib.kyhip_pass_boundaries(int(spp), out, n)
    return list(out)


def slice_bounds(spp, n):
    """kyhip_slice_bounds (host only): n + 1 ascending pass boundaries from 0 to spp that cut an spp-sample frame into n slices of about equal sample counts;
    slice k owns samples [bounds[k], bounds[k + 1])."""
    lib = A.load_kyhip()
    out = (C.c_int * (max(int(n), 0) + 1))()
    _check(lib.kyhip_slice_bounds(int(spp), int(n), out), lib)
    return list(out)


def denoise_defaults():
    """kyhip_denoise_defaults (host only) as a ky_denoise_params (_abi.DenoiseParams)."""
    q = A.DenoiseParams()
    A.load_kyhip().kyhip_denoise_defaults(C.byref(q))
    return q


def temporal_defaults():
    """kyhip_temporal_defaults (host only) as a ky_temporal_params (_abi.TemporalParams)."""
    t = A.TemporalParams()
    A.load_kyhip().kyhip_temporal_defaults(C.byref(t))
    return t


class History:
    """What frames of ONE scene under a moving camera hand to each other (kyhip_history_*): `with History(w, h) as hist: ... f.denoise(history=hist)` for frame
    after frame.  Per pixel the accumulated colour, variance and sample count, the guides and the camera of the frame that wrote them; on the device, independent
    of any frame's lifetime, no part of a checkpoint.  The scene being the same but for the camera is the caller's contract.  reset(): it holds no picture
    afterwards; frames: the temporal calls since; read(): ((H, W, 4) {r, g, b, v}, (H, W) counts); ms(): the last temporal kernel's span."""

    def __init__(self, width, height, device=0):
        self._lib = A.load_kyhip()
        self._h = C.c_void_p()
        self.width, self.height = int(width), int(height)
        _check(self._lib.kyhip_history_create(int(device), self.width, self.height, C.byref(self._h)), self._lib)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.kyhip_history_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def reset(self):
        _check(self._lib.kyhip_history_reset(self._h), self._lib)

    @property
    def frames(self):
        n = self._lib.kyhip_history_frames(self._h)
        if n < 0:
            _check(n, self._lib)
        return n

    def read(self):
        cv, m = np.zeros((self.height, self.width, 4), np.float32), np.zeros((self.height, self.width), np.float32)
        _check(self._lib.kyhip_history_read(self._h, C.c_void_p(cv.ctypes.data), C.c_void_p(m.ctypes.data), self.width), self._lib)
        return cv, m

    def ms(self):
        a = C.c_float(-1)
        _check(self._lib.kyhip_history_ms(self._h, C.byref(a)), self._lib)
        return a.value


class Frame:
    """A frame rendered in passes (kyhip_frame_*): `with Frame(scene, params) as f: f.render(64); preview = f.resolve(normalise=True); ...`.
    params.samples_per_pixel is the frame's total; a complete frame's resolve() is render(scene, params), bit for bit.
    noise=True: the frame keeps a per-pixel noise estimate over its passes (kyhip_frame_track_noise): noise(), noise_stats(threshold), render_until(...).
    blocks=True: the frame retires 8 x 8 pixel blocks between its passes and renders the live ones only (kyhip_frame_track_blocks): keep(mask),
    retire_noisy(...) and render_adaptive(...) (these two with noise=True), sample_map(), block_stats(); resolve(normalise=True) is then per block.
    A frame with noise=True whose shard is the whole film can be denoised between passes: denoise(), guides(), denoise_ms().
    guide_bounces=1 .. 4: the denoiser's guides follow mirrors and glass for that many specular vertices behind the first hit, and a pixel's taps are the pixels
    with the same chain (guide_chains()); 0, the default: first-hit guides.  A win at preview sample counts on the Cornell box with its two balls, mixed at 224
    samples and more and behind a large curved mirror (DESIGN.md "Denoise").
    slice=(first, end): the frame owns and renders samples [first, end) of every pixel only (kyhip_frame_begin_slice; both 0 or a pass boundary, see slice_bounds);
    first == end is a collector that renders nothing.  merge() adds what another frame of the same scene and params holds, bit for bit: `done` counts the samples
    held, `coverage` lists them, and slices that cover 0 .. total merged into one of them resolve to render(scene, params).
    filter=pixel_filter(...): the frame's camera samples are drawn from the filter's density (kyhip_frame_set_filter); a complete frame's resolve() is then
    render(scene, params, filter=filter) bit for bit, and its states load and merge only into frames with the same filter.
    lens=lens(...): the frame's camera rays leave from that lens (kyhip_frame_set_lens), with the same two consequences.
    albedo=G, 1 .. 8: denoise() divides every surface pixel by an albedo before its levels and multiplies it back behind them (kyhip_frame_set_albedo_grid): the
    mean colour of what G x G camera rays per pixel end on, the frame's textures included, traced once per frame with the guides (albedo(), albedo_ms()); 0, the
    default: off, and denoise() is what it is without."""

    def __init__(self, scene, params, device=0, noise=False, blocks=False, slice=None, guide_bounces=0, filter=None, lens=None, textures=None, albedo=0):
        self._lib = A.load_kyhip()
        self._f = C.c_void_p()
        self.height, self.width = params.height, params.width
        if slice is None:
            _check(self._lib.kyhip_frame_begin(device, _scene_ptr(scene), C.byref(params), C.byref(self._f)), self._lib)
        else:
            _check(self._lib.kyhip_frame_begin_slice(device, _scene_ptr(scene), C.byref(params), int(slice[0]), int(slice[1]), C.byref(self._f)), self._lib)
        if noise:
            rc = self._lib.kyhip_frame_track_noise(self._f)
            if rc != A.KY_OK:
                self.close()
                _check(rc, self._lib)
        if blocks:
            rc = self._lib.kyhip_frame_track_blocks(self._f)
            if rc != A.KY_OK:
                self.close()
                _check(rc, self._lib)
        if guide_bounces:
            rc = self._lib.kyhip_frame_set_guide_bounces(self._f, int(guide_bounces))
            if rc != A.KY_OK:
                self.close()
                _check(rc, self._lib)
        if albedo:
            rc = self._lib.kyhip_frame_set_albedo_grid(self._f, int(albedo))
            if rc != A.KY_OK:
                self.close()
                _check(rc, self._lib)
        if filter is not None:
            rc = self._lib.kyhip_frame_set_filter(self._f, C.byref(filter))
            if rc != A.KY_OK:
                self.close()
                _check(rc, self._lib)

        if lens is not None:
            rc = self._lib.kyhip_frame_set_lens(self._f, C.byref(lens))
            if rc != A.KY_OK:
                self.close()
                _check(rc, self._lib)

        if textures:   # textures=[texture_checker(...), texture_image(...)]: kyhip_frame_set_textures, part of what the frame is, like its filter and lens
            try:
                self.set_textures(textures)
            except KyError:
                self.close()
                raise

    def set_textures(self, textures):
        """kyhip_frame_set_textures: the frame's texture set, copied and uploaded once; refused once the frame holds a sample."""
        arr, n = _texture_array(textures)
        _check(self._lib.kyhip_frame_set_textures(self._f, arr, n), self._lib)

    def set_lens(self, lens):
        """kyhip_frame_set_lens: the frame's lens; refused once the frame holds a sample."""
        _check(self._lib.kyhip_frame_set_lens(self._f, C.byref(lens)), self._lib)

    @property
    def lens(self):
        """kyhip_frame_lens: the frame's lens (the pinhole, radius 0, until one is set)."""
        l = A.Lens()
        _check(self._lib.kyhip_frame_lens(self._f, C.byref(l)), self._lib)
        return l

    def set_filter(self, filter):
        """kyhip_frame_set_filter: the frame's pixel filter; refused once the frame holds a sample."""
        _check(self._lib.kyhip_frame_set_filter(self._f, C.byref(filter)), self._lib)

    @property
    def filter(self):
        """kyhip_frame_filter: the frame's pixel filter (the box until one is set)."""
        f = A.PixelFilter()
        _check(self._lib.kyhip_frame_filter(self._f, C.byref(f)), self._lib)
        return f

    def set_guide_bounces(self, bounces):
        """kyhip_frame_set_guide_bounces: 0 .. 4 specular vertices the denoiser's guides follow behind the first hit; refused once the guides are traced."""
        _check(self._lib.kyhip_frame_set_guide_bounces(self._f, int(bounces)), self._lib)

    @property
    def guide_bounces(self):
        n = self._lib.kyhip_frame_guide_bounces(self._f)
        if n < 0:
            _check(n, self._lib)
        return n

    def set_albedo_grid(self, grid):
        """kyhip_frame_set_albedo_grid: 0 (off) .. 8 sub-samples per pixel edge of the albedo denoise() demodulates by; refused once the guides are traced."""
        _check(self._lib.kyhip_frame_set_albedo_grid(self._f, int(grid)), self._lib)

    @property
    def albedo_grid(self):
        n = self._lib.kyhip_frame_albedo_grid(self._f)
        if n < 0:
            _check(n, self._lib)
        return n

    def close(self):
        if getattr(self, "_f", None):
            self._lib.kyhip_frame_end(self._f)
            self._f = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _samples(self):
        done, total = C.c_int(0), C.c_int(0)
        _check(self._lib.kyhip_frame_samples(self._f, C.byref(done), C.byref(total)), self._lib)
        return done.value, total.value

    @property
    def done(self):
        return self._samples()[0]

    @property
    def total(self):
        return self._samples()[1]

    def render(self, min_samples):
        """One pass: whole chunks until at least min_samples more samples per pixel are done, or the frame is complete; returns the samples done so far."""
        done = C.c_int(0)
        _check(self._lib.kyhip_frame_render(self._f, int(min_samples), C.byref(done)), self._lib)
        return done.value

    def resolve(self, normalise=False, film=None, row_stride_px=None, origin_px=(0, 0)):
        """ADDS the picture to `film` (a new zero film by default) and returns it: sum / total, or with normalise the mean of the samples done so far."""
        if film is None:
            film = np.zeros((self.height, self.width, 3), np.float32)
        stride = film.shape[1] if row_stride_px is None else row_stride_px
        base = film.ctypes.data + (origin_px[1] * stride + origin_px[0]) * 12
        _check(self._lib.kyhip_frame_resolve(self._f, 1 if normalise else 0, C.c_void_p(base), stride), self._lib)
        return film

    def save(self):
        """The frame's checkpoint as bytes (kyhip_frame_save)."""
        n = self._lib.kyhip_frame_state_bytes(self._f)
        if n < 0:
            _check(n, self._lib)
        buf = C.create_string_buffer(n)
        _check(self._lib.kyhip_frame_save(self._f, buf, n), self._lib)
        return buf.raw

    def noise(self, out=None):
        """The (H, W) float32 noise map (kyhip_frame_noise): per pixel of the frame's shard the standard error of its mean luminance so far, in units of the
        film's white; +inf before the second pass, 0 for flagged pixels.  Pixels of other shards keep `out`'s values (a new map: 0)."""
        if out is None:
            out = np.zeros((self.height, self.width), np.float32)
        assert out.dtype == np.float32 and out.shape == (self.height, self.width) and out.strides[1] == 4 and out.strides[0] % 4 == 0
        _check(self._lib.kyhip_frame_noise(self._f, C.c_void_p(out.ctypes.data), out.strides[0] // 4), self._lib)
        return out

    def noise_stats(self, threshold):
        """kyhip_frame_noise_stats as a ky_noise_stats (_abi.NoiseStats): batches, samples_done, pixels, flagged, above, threshold, max, mean."""
        st = A.NoiseStats()
        _check(self._lib.kyhip_frame_noise_stats(self._f, float(threshold), C.byref(st)), self._lib)
        return st

    def render_until(self, threshold, max_fraction_above=0.0, min_batches=2, min_samples_per_pass=1):
        """Passes until at most max_fraction_above of the pixels are noisier than threshold (after min_batches passes or more) or the frame is complete:
        (samples done, the statistics behind the last pass)."""
        done, st = C.c_int(0), A.NoiseStats()
        _check(self._lib.kyhip_frame_render_until(self._f, float(threshold), float(max_fraction_above), int(min_batches), int(min_samples_per_pass),
                                                  C.byref(done), C.byref(st)), self._lib)
        return done.value, st

    def keep(self, mask):
        """kyhip_frame_keep: retires every live block none of whose in-film pixels is set in the (H, W) mask (bool or uint8)."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        assert m.shape == (self.height, self.width)
        _check(self._lib.kyhip_frame_keep(self._f, C.c_void_p(m.ctypes.data), m.strides[0]), self._lib)

    def retire_noisy(self, threshold, max_fraction_above=0.0, min_batches=2):
        """kyhip_frame_retire_noisy: the retire rule applied once to the live blocks; returns the ky_block_stats (_abi.BlockStats) behind it."""
        st = A.BlockStats()
        _check(self._lib.kyhip_frame_retire_noisy(self._f, float(threshold), float(max_fraction_above), int(min_batches), C.byref(st)), self._lib)
        return st

    def render_adaptive(self, threshold, max_fraction_above=0.0, min_batches=2, min_samples_per_pass=1):
        """Passes, each followed by the retire rule, until no block is live or the frame's front reaches the total: (the front, the block statistics)."""
        done, st = C.c_int(0), A.BlockStats()
        _check(self._lib.kyhip_frame_render_adaptive(self._f, float(threshold), float(max_fraction_above), int(min_batches), int(min_samples_per_pass),
                                                     C.byref(done), C.byref(st)), self._lib)
        return done.value, st

    def sample_map(self, out=None):
        """The (H, W) int32 map of the samples each pixel's block has received (kyhip_frame_sample_map); other shards' pixels keep `out`'s values (new: 0)."""
        if out is None:
            out = np.zeros((self.height, self.width), np.int32)
        assert out.dtype == np.int32 and out.shape == (self.height, self.width) and out.strides[1] == 4 and out.strides[0] % 4 == 0
        _check(self._lib.kyhip_frame_sample_map(self._f, C.c_void_p(out.ctypes.data), out.strides[0] // 4), self._lib)
        return out

    def blocks_ms(self):
        """kyhip_frame_blocks_ms: (the last retire / keep kernel, the last compaction of the live list) in ms, negative where there was none."""
        a, b = C.c_float(-1), C.c_float(-1)
        _check(self._lib.kyhip_frame_blocks_ms(self._f, C.byref(a), C.byref(b)), self._lib)
        return a.value, b.value

    def block_stats(self):
        """kyhip_frame_block_stats as a ky_block_stats (_abi.BlockStats)."""
        st = A.BlockStats()
        _check(self._lib.kyhip_frame_block_stats(self._f, C.byref(st)), self._lib)
        return st

    def denoise(self, params=None, film=None, row_stride_px=None, origin_px=(0, 0), history=None, temporal=None):
        """ADDS the denoised picture so far to `film` (a new zero film by default) and returns it (kyhip_frame_denoise): resolve(normalise=True) through an
        edge-avoiding a-trous filter guided by the frame's variance estimate and its first-hit geometry (guide_bounces: the geometry its specular chains end on).  params: a ky_denoise_params (_abi.DenoiseParams) or a dict
        of its fields over denoise_defaults(); None: the defaults.  levels=0 is resolve(normalise=True).
        history=History(...): kyhip_frame_denoise_temporal -- before the levels every surface pixel is blended with what the history's frames of the same scene
        saw of its point, and the history takes the result; temporal: a ky_temporal_params (_abi.TemporalParams) or a dict of its fields over
        temporal_defaults().  levels=0 then delivers the accumulated picture unfiltered."""
        if isinstance(params, dict):
            q = denoise_defaults()
            for name, value in params.items():
                setattr(q, name, value)
            params = q
        if isinstance(temporal, dict):
            t = temporal_defaults()
            for name, value in temporal.items():
                setattr(t, name, value)
            temporal = t
        if history is None and temporal is not None:
            raise ValueError("temporal parameters without a history")
        if film is None:
            film = np.zeros((self.height, self.width, 3), np.float32)
        stride = film.shape[1] if row_stride_px is None else row_stride_px
        base = film.ctypes.data + (origin_px[1] * stride + origin_px[0]) * 12
        if history is None:
            _check(self._lib.kyhip_frame_denoise(self._f, None if params is None else C.byref(params), C.c_void_p(base), stride), self._lib)
        else:
            _check(self._lib.kyhip_frame_denoise_temporal(self._f, history._h, None if params is None else C.byref(params),
                                                          None if temporal is None else C.byref(temporal), C.c_void_p(base), stride), self._lib)
        return film

    def guides(self):
        """kyhip_frame_guides: ((H, W, 4) {n.x, n.y, n.z, t}, (H, W, 4) {P.x, P.y, P.z, class}) float32 of the camera rays through the pixel centres; class 0
        surface, 1 miss, 2 a surface that carries an area light, 3 flagged.  With guide_bounces: of the vertex the pixel's specular chain ends on, t summed
        along the chain (an unresolved chain: the first hit's)."""
        a, b = np.zeros((self.height, self.width, 4), np.float32), np.zeros((self.height, self.width, 4), np.float32)
        _check(self._lib.kyhip_frame_guides(self._f, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), self.width), self._lib)
        return a, b

    def guide_chains(self):
        """kyhip_frame_guide_chains: the (H, W) uint64 chain keys: 10 bits per specular vertex k at bit 10 k, ((surface + 1) << 1) | (1 if transmitted); 0 where
        the first hit is neither mirror nor glass (everywhere at guide_bounces=0); bit 62 (_abi.GUIDE_KEY_UNRESOLVED) plus the first digit where the chain
        has more specular vertices than guide_bounces."""
        keys = np.zeros((self.height, self.width), np.uint64)
        _check(self._lib.kyhip_frame_guide_chains(self._f, C.c_void_p(keys.ctypes.data), self.width), self._lib)
        return keys

    def albedo(self):
        """kyhip_frame_albedo: (H, W, 4) float32 {r, g, b, w}: the albedo a frame with an albedo grid demodulates by, and the number of the pixel's sub-samples
        that ended on a surface without a lamp."""
        a = np.zeros((self.height, self.width, 4), np.float32)
        _check(self._lib.kyhip_frame_albedo(self._f, C.c_void_p(a.ctypes.data), self.width), self._lib)
        return a

    def albedo_ms(self):
        """kyhip_frame_albedo_ms: the albedo trace in ms, negative where there was none."""
        a = C.c_float(-1)
        _check(self._lib.kyhip_frame_albedo_ms(self._f, C.byref(a)), self._lib)
        return a.value

    def denoise_ms(self):
        """kyhip_frame_denoise_ms: (the guide trace, the last denoise()'s gather + levels + add) in ms, negative where there was none."""
        a, b = C.c_float(-1), C.c_float(-1)
        _check(self._lib.kyhip_frame_denoise_ms(self._f, C.byref(a), C.byref(b)), self._lib)
        return a.value, b.value

    def _coverage(self):
        ranges, own = (C.c_int * (2 * A.SLICE_MAX_RANGES))(), (C.c_int * 2)()
        n = self._lib.kyhip_frame_coverage(self._f, ranges, A.SLICE_MAX_RANGES, own)
        if n < 0:
            _check(n, self._lib)
        return [(ranges[2 * i], ranges[2 * i + 1]) for i in range(n)], (own[0], own[1])

    @property
    def coverage(self):
        """The sample ranges [(first, end), ...] the frame holds: ascending, disjoint, adjacent ones joined (kyhip_frame_coverage)."""
        return self._coverage()[0]

    @property
    def own(self):
        """The sample range (first, end) the frame owns and renders."""
        return self._coverage()[1]

    def merge(self, other):
        """Adds what another frame of the same scene and params holds -- a Frame of this process (kyhip_frame_merge_from: no host round trip) or the bytes its
        save() returned, from any device, process or machine (kyhip_frame_merge).  Its samples must be disjoint from this frame's coverage and owned range."""
        if isinstance(other, Frame):
            _check(self._lib.kyhip_frame_merge_from(self._f, other._f), self._lib)
        else:
            state = bytes(other)
            _check(self._lib.kyhip_frame_merge(self._f, state, len(state)), self._lib)

    def merge_ms(self):
        """kyhip_frame_merge_ms: the last merge kernel in ms, negative when there was none."""
        ms = C.c_float(-1)
        _check(self._lib.kyhip_frame_merge_ms(self._f, C.byref(ms)), self._lib)
        return ms.value

    def load(self, state):
        """Continue from a checkpoint of a frame begun with the same scene and params (kyhip_frame_load); any other state raises KyError."""
        state = bytes(state)
        _check(self._lib.kyhip_frame_load(self._f, state, len(state)), self._lib)


def render_sliced(scene, params, devices, min_samples_per_pass, on_pass=None, noise=False, film=None, filter=None, lens=None, textures=None):
    """The frame in len(devices) slices of its samples (slice_bounds), slice k on devices[k] (a device may repeat); returns the (accumulated) host film, which is
    render(scene, params) bit for bit.  The slices render in rounds of one pass each, one call after the other (concurrency across devices: ky_amd.dist); after
    every round on_pass(done, total, preview) is called with the samples per pixel done over all slices, and preview(denoise=False) merges the slices as they stand
    into a collector and returns its picture: resolve(normalise=True), or with denoise=True (needs noise=True and two rounds) denoise().  At the end slice 0's
    frame merges the others and resolves.  filter, lens: every slice's (and the collector's) pixel filter and lens; the film is then render(scene, params, filter=filter, lens=lens).
    textures: likewise every slice's texture set."""
    bounds = slice_bounds(params.samples_per_pixel, len(devices))
    frames = []
    try:
        for k, dev in enumerate(devices):
            frames.append(Frame(scene, params, device=dev, noise=noise, slice=(bounds[k], bounds[k + 1]), filter=filter, lens=lens, textures=textures))

        def preview(denoise=False):
            with Frame(scene, params, device=devices[0], noise=noise, slice=(0, 0), filter=filter, lens=lens, textures=textures) as collector:
                for f in frames:
                    collector.merge(f)
                return collector.denoise() if denoise else collector.resolve(normalise=True)

        while any(f.done < f.own[1] - f.own[0] for f in frames):
            for f in frames:
                f.render(min_samples_per_pass)
            if on_pass is not None:
                on_pass(sum(f.done for f in frames), params.samples_per_pixel, preview)
        for f in frames[1:]:
            frames[0].merge(f)
        return frames[0].resolve(film=film)
    finally:
        for f in frames:
            f.close()


class PinnedFilm:
    """A [height, width, 3] float32 numpy view of pinned host memory from kyhip_film_alloc (include/kyhip.h): a film the GPU adds to in place.
    `array` stays valid while this object lives."""

    def __init__(self, height, width):
        lib = A.load_kyhip()
        self._lib, self.nbytes = lib, height * width * 12
        self._ptr = lib.kyhip_film_alloc(self.nbytes)
        if not self._ptr:
            raise MemoryError("kyhip_film_alloc returned NULL (no device?)")
        self.array = np.ctypeslib.as_array((C.c_float * (height * width * 3)).from_address(self._ptr)).reshape(height, width, 3)
        self.array[...] = 0

    def __del__(self):
        if getattr(self, "_ptr", None):
            self.array = None
            self._lib.kyhip_film_free(self._ptr)
            self._ptr = None


def render_multi(scene, params, devices, film=None, row_stride_px=None, origin_px=(0, 0)):
    """kyhip_render_multi: integrator_t::render with the frame's tiles spread over the listed GPUs (a device may repeat)."""
    lib = A.load_kyhip()
    if film is None:
        film = np.zeros((params.height, params.width, 3), np.float32)
    stride = film.shape[1] if row_stride_px is None else row_stride_px
    base = film.ctypes.data + (origin_px[1] * stride + origin_px[0]) * 12
    devs = (C.c_int * len(devices))(*devices)
    _check(lib.kyhip_render_multi(devs, len(devices), _scene_ptr(scene), C.byref(params), C.c_void_p(base), stride))
    return film


def render_host_api(scene, integrator_enum, depth, direct_sample, sampler, spp, width, height, seed=1234,
                    grid=None, cell=0, film=None, device=0, lighting=None):
    """Drive the C++ host classes exactly like a reference driver: create_integrator(...)->render(&scene, sampler, &film).
    lighting: integrator->set_lighting(lighting) first (lighting_enum_t: the light classes render() adds)."""
    host = A.load_kyhost()
    rows, cols = grid if grid else (0, 0)
    fw, fh = (cols * width, rows * height) if grid else (width, height)
    if film is None:
        film = np.zeros((fh, fw, 3), np.float32)
    if lighting is None:
        rc = host.kyhost_render(scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, rows, cols,
                                cell, _fptr(film), device)
    else:
        rc = host.kyhost_render_lighting(scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, rows, cols,
                                         cell, _fptr(film), device, int(lighting))
    if rc == -2:
        return None  # create_integrator returned nullptr (ky.cpp:4638)
    if rc != 0:
        raise KyError("kyhost_render failed: " + host.kyhost_last_error().decode())
    return film


def render_passes_host_api(scene, integrator_enum, depth, direct_sample, sampler, spp, width, height, min_samples_per_pass, on_pass=None, seed=1234,
                           film=None, device=0):
    """create_integrator(...)->render_passes(&scene, sampler, &film, min_samples_per_pass, on_pass) through the C++ host classes: on_pass(done, total)
    is called after every pass and stops the frame by returning False (the film then gets the mean of the samples done)."""
    host = A.load_kyhost()
    if film is None:
        film = np.zeros((height, width, 3), np.float32)
    cb_type = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.c_void_p)
    cb = cb_type(lambda done, total, _user: 1 if on_pass(done, total) else 0) if on_pass else C.cast(None, cb_type)
    rc = host.kyhost_render_passes(scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, _fptr(film), device,
                                   int(min_samples_per_pass), C.cast(cb, C.c_void_p), None)
    if rc == -2:
        return None
    if rc != 0:
        raise KyError("kyhost_render_passes failed: " + host.kyhost_last_error().decode())
    return film


def render_filtered_host_api(scene, integrator_enum, depth, direct_sample, sampler, spp, width, height, filter, mode="render", min_samples_per_pass=4, seed=1234,
                             film=None, device=0):
    """film_t::set_filter(filter) then create_integrator(...)->render / render_passes / render_sliced (over the device twice) / render_until (with a threshold
    nothing reaches) through the C++ host classes (ky.hpp, filter_t): mode "render", "passes", "sliced" or "until".  filter: a pixel_filter(...)."""
    host = A.load_kyhost()
    if film is None:
        film = np.zeros((height, width, 3), np.float32)
    rc = host.kyhost_render_filtered(scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, _fptr(film), device, int(filter.kind),
                                     float(filter.radius), float(filter.param), ("render", "passes", "sliced", "until").index(mode), int(min_samples_per_pass))
    if rc == -2:
        return None
    if rc != 0:
        raise KyError("kyhost_render_filtered failed: " + host.kyhost_last_error().decode())
    return film


def render_lens_host_api(scene, integrator_enum, depth, direct_sample, sampler, spp, width, height, lens, mode="render", min_samples_per_pass=4, seed=1234, film=None,
                         device=0):
    """camera_t::set_lens(radius, focus_distance) on the scene's camera, then create_integrator(...)->render / render_passes / render_sliced (over the device twice)
    through the C++ host classes (ky.hpp): mode "render", "passes" or "sliced".  The scene's camera is the pinhole again afterwards.  lens: a lens(...)."""
    host = A.load_kyhost()
    if film is None:
        film = np.zeros((height, width, 3), np.float32)
    rc = host.kyhost_render_lens(scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, _fptr(film), device, float(lens.radius),
                                 float(lens.focus_distance), ("render", "passes", "sliced").index(mode), int(min_samples_per_pass))
    if rc == -2:
        return None
    if rc != 0:
        raise KyError("kyhost_render_lens failed: " + host.kyhost_last_error().decode())
    return film


def render_sliced_host_api(scene, integrator_enum, depth, direct_sample, sampler, spp, width, height, devices, min_samples_per_pass, seed=1234, film=None):
    """create_integrator(...)->render_sliced(&scene, sampler, &film, devices, min_samples_per_pass) through the C++ host classes: the frame by sample range, slice k
    on devices[k], merged on devices[0]; returns the film (render_host_api's, bit for bit)."""
    host = A.load_kyhost()
    if film is None:
        film = np.zeros((height, width, 3), np.float32)
    devs = (C.c_int * len(devices))(*devices)
    rc = host.kyhost_render_sliced(scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, _fptr(film), devs, len(devices),
                                   int(min_samples_per_pass))
    if rc == -2:
        return None
    if rc != 0:
        raise KyError("kyhost_render_sliced failed: " + host.kyhost_last_error().decode())
    return film


def render_until_host_api(scene, integrator_enum, depth, direct_sample, sampler, spp, width, height, threshold, max_fraction_above=0.0, min_batches=2,
                          min_samples_per_pass=1, seed=1234, film=None, device=0):
    """create_integrator(...)->render_until(&scene, sampler, &film, threshold, max_fraction_above, min_batches, min_samples_per_pass) through the C++ host
    classes: (the film with the mean of the samples done added, the samples done per pixel)."""
    host = A.load_kyhost()
    if film is None:
        film = np.zeros((height, width, 3), np.float32)
    rc = host.kyhost_render_until(scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, _fptr(film), device,
                                  float(threshold), float(max_fraction_above), int(min_batches), int(min_samples_per_pass))
    if rc == -2:
        return None
    if rc < 0:
        raise KyError("kyhost_render_until failed: " + host.kyhost_last_error().decode())
    return film, rc


def render_adaptive_host_api(scene, integrator_enum, depth, direct_sample, sampler, spp, width, height, threshold, max_fraction_above=0.0, min_batches=2,
                             min_samples_per_pass=1, seed=1234, film=None, device=0):
    """create_integrator(...)->render_adaptive(&scene, sampler, &film, threshold, max_fraction_above, min_batches, min_samples_per_pass, &counts) through the
    C++ host classes: (the film with each block's mean added, the (H, W) int32 sample counts, the ky_block_stats)."""
    host = A.load_kyhost()
    if film is None:
        film = np.zeros((height, width, 3), np.float32)
    counts = np.zeros((height, width), np.int32)
    st = A.BlockStats()
    rc = host.kyhost_render_adaptive(scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, _fptr(film), device,
                                     float(threshold), float(max_fraction_above), int(min_batches), int(min_samples_per_pass), C.c_void_p(counts.ctypes.data),
                                     C.byref(st))
    if rc == -2:
        return None
    if rc != 0:
        raise KyError("kyhost_render_adaptive failed: " + host.kyhost_last_error().decode())
    return film, counts, st


def render_denoised_host_api(scene, integrator_enum, depth, direct_sample, sampler, spp, width, height, min_samples_per_pass, stop_after_samples, params=None,
                             seed=1234, film=None, device=0, guide_bounces=None, albedo=None):
    """create_integrator(...)->render_denoised(&scene, sampler, &film, min_samples_per_pass, stop_after_samples, params) through the C++ host classes: (the film
    with the denoised picture so far added, the samples done per pixel).  params: an _abi.DenoiseParams, None for the library's defaults.  guide_bounces: None,
    or render_denoised's guide_bounces (kyhost_render_denoised_chains).  albedo: None, or render_denoised's albedo_grid (kyhost_render_denoised_albedo)."""
    host = A.load_kyhost()
    if film is None:
        film = np.zeros((height, width, 3), np.float32)
    args = (scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, _fptr(film), device, int(min_samples_per_pass),
            int(stop_after_samples), None if params is None else C.byref(params))
    if albedo is not None:
        rc = host.kyhost_render_denoised_albedo(*args, int(guide_bounces or 0), int(albedo))
    else:
        rc = host.kyhost_render_denoised(*args) if guide_bounces is None else host.kyhost_render_denoised_chains(*args, int(guide_bounces))
    if rc == -2:
        return None
    if rc < 0:
        raise KyError("kyhost_render_denoised failed: " + host.kyhost_last_error().decode())
    return film, rc


def debug_area_host_api(scene, integrator_enum, depth, direct_sample, sampler, spp, width, height, begin, end, film=None, seed=1234, device=0):
    """create_integrator(...)->debug_area(&scene, sampler, &film, begin, end) (ky.cpp:3733-3777) through the C++ host classes; a 1 x 1 area
    goes through debug_pixel (3784).  Returns the film (modified in place when given)."""
    host = A.load_kyhost()
    if film is None:
        film = np.zeros((height, width, 3), np.float32)
    rc = host.kyhost_debug_area(scene.ptr, integrator_enum, depth, direct_sample, sampler, spp, seed, width, height, _fptr(film),
                                int(begin[0]), int(begin[1]), int(end[0]), int(end[1]), device)
    if rc == -2:
        return None
    if rc != 0:
        raise KyError("kyhost_debug_area failed: " + host.kyhost_last_error().decode())
    return film


def kernel_ms(device=0):
    return float(A.load_kyhip().kyhip_kernel_ms(device))


# ---- function-level entry points (parity tests) -------------------------------------------------

def kat_intersect(shape, rays7, device=0):
    lib = A.load_kyhip()
    rays7 = np.ascontiguousarray(rays7, np.float32)
    out = np.zeros((rays7.shape[0], 8), np.float32)
    _check(lib.kyhip_kat_intersect(device, C.byref(shape), _fptr(rays7), rays7.shape[0], _fptr(out)))
    return out


def kat_camera(camera, p_film2, device=0):
    lib = A.load_kyhip()
    p_film2 = np.ascontiguousarray(p_film2, np.float32)
    out = np.zeros((p_film2.shape[0], 6), np.float32)
    _check(lib.kyhip_kat_camera(device, C.byref(camera), _fptr(p_film2), p_film2.shape[0], _fptr(out)))
    return out


def kat_bsdf(material, in12, device=0):
    lib = A.load_kyhip()
    in12 = np.ascontiguousarray(in12, np.float32)
    out = np.zeros((in12.shape[0], 13), np.float32)
    _check(lib.kyhip_kat_bsdf(device, C.byref(material), _fptr(in12), in12.shape[0], _fptr(out)))
    return out


def kat_bsdf_continue(material, in12, flat_phong=False, device=0):
    """kyhip_kat_bsdf_continue: kat_bsdf's rows through the render kernels' lobe code -> n x {wi[3], weight[3], ok, specular, col * scale [3], pdf}."""
    lib = A.load_kyhip()
    in12 = np.ascontiguousarray(in12, np.float32)
    out = np.zeros((in12.shape[0], 12), np.float32)
    _check(lib.kyhip_kat_bsdf_continue(device, C.byref(material), _fptr(in12), in12.shape[0], 1 if flat_phong else 0, _fptr(out)))
    return out


def kat_light(scene, light, in11, device=0):
    lib = A.load_kyhip()
    in11 = np.ascontiguousarray(in11, np.float32)
    out = np.zeros((in11.shape[0], 11), np.float32)
    _check(lib.kyhip_kat_light(device, _scene_ptr(scene), light, _fptr(in11), in11.shape[0], _fptr(out)))
    return out


def kat_scene_intersect(scene, rays7, device=0):
    lib = A.load_kyhip()
    rays7 = np.ascontiguousarray(rays7, np.float32)
    out = np.zeros((rays7.shape[0], 9), np.float32)
    _check(lib.kyhip_kat_scene_intersect(device, _scene_ptr(scene), _fptr(rays7), rays7.shape[0], _fptr(out)))
    return out


def kat_any_pair(scene, in13, device=0):
    """trace_any_pair (the environment estimate's scan): n x {o_a, d_a, o_b, d_b, tmax_b} -> n x {A meets a surface, B meets one before tmax_b}."""
    lib = A.load_kyhip()
    in13 = np.ascontiguousarray(in13, np.float32)
    out = np.zeros((in13.shape[0], 2), np.float32)
    _check(lib.kyhip_kat_any_pair(device, _scene_ptr(scene), _fptr(in13), in13.shape[0], _fptr(out)))
    return out


def kat_occluded(scene, in9, device=0, table=None):
    """scene_t::occluded for n x {p, normal, target}.  table None: every surface is tested; -1 / a light index: the occluder table the
    render kernels use for segments between scene points / for shadow rays towards samples of that light (kyhip_kat_occluded_between)."""
    lib = A.load_kyhip()
    in9 = np.ascontiguousarray(in9, np.float32)
    out = np.zeros((in9.shape[0],), np.float32)
    if table is None:
        _check(lib.kyhip_kat_occluded(device, _scene_ptr(scene), _fptr(in9), in9.shape[0], _fptr(out)))
    else:
        _check(lib.kyhip_kat_occluded_between(device, _scene_ptr(scene), int(table), _fptr(in9), in9.shape[0], _fptr(out)))
    return out


def scene_non_occluders(scene, light=-1):
    """kyhip_scene_non_occluders (host only), per surface: 1 not in the occluder table for `light` (-1: rays that end on a scene point),
    2 scanned only for rays with an end behind that light's plane, 0 always tested."""
    lib = A.load_kyhip()
    n = _scene_ptr(scene).contents.surface_count
    out = np.zeros(max(1, n), np.int32)
    rc = lib.kyhip_scene_non_occluders(_scene_ptr(scene), int(light), out.ctypes.data_as(C.c_void_p), n)
    if rc < 0:
        _check(rc)
    return out[:n].copy()


def scene_facts(scene):
    """kyhip_scene_facts (host only): the KY_FEAT_* mask the library finds for the scene."""
    lib = A.load_kyhip()
    rc = lib.kyhip_scene_facts(_scene_ptr(scene))
    if rc < 0:
        _check(rc)
    return rc


def scene_boxes(scene):
    """kyhip_scene_boxes (host only): (number of boxes, per surface 8 * box + 2 * axis + side for a surface that is a whole face of an axis-aligned box
    the nearest-hit traversal tests with one slab test, -1 otherwise)."""
    lib = A.load_kyhip()
    n = _scene_ptr(scene).contents.surface_count
    out = np.zeros(max(1, n), np.int32)
    rc = lib.kyhip_scene_boxes(_scene_ptr(scene), out.ctypes.data_as(C.c_void_p), n)
    if rc < 0:
        _check(rc)
    return rc, out[:n].copy()


def scene_screen_bound(scene, params, filter=None, lens=None):
    """kyhip_scene_screen_bound (host only): ((x0, y0, x1, y1), dead, total) -- the scene's live rectangle in the frame of `params` (no camera ray of a pixel outside it
    reaches a surface), and the 8 x 8 blocks of the params' shard outside it / in all.  filter: kyhip_scene_screen_bound_filtered -- the rectangle a launch under
    that pixel filter reads, grown by ceil(radius - 0.5) pixels on every side.  lens: kyhip_scene_screen_bound_lens -- with radius > 0 the whole frame, nothing dead."""
    lib = A.load_kyhip()
    rect = (C.c_int * 4)()
    counts = (C.c_longlong * 2)()
    if lens is not None:
        _check(lib.kyhip_scene_screen_bound_lens(_scene_ptr(scene), C.byref(params), C.byref(filter) if filter is not None else None, C.byref(lens), rect, counts))
    elif filter is None:
        _check(lib.kyhip_scene_screen_bound(_scene_ptr(scene), C.byref(params), rect, counts))
    else:
        _check(lib.kyhip_scene_screen_bound_filtered(_scene_ptr(scene), C.byref(params), C.byref(filter), rect, counts))
    return tuple(int(v) for v in rect), int(counts[0]), int(counts[1])


def kat_li(scene, params, x, y, s0, n, device=0, filter=None, lens=None, textures=None):
    lib = A.load_kyhip()
    out = np.zeros((n, 3), np.float32)
    if textures:   # kyhip_kat_li_textured: the samples of a render under that texture set (and pixel filter and lens)
        arr, nt = _texture_array(textures)
        _check(lib.kyhip_kat_li_textured(device, _scene_ptr(scene), arr, nt, C.byref(params), C.byref(filter) if filter is not None else None,
                                         C.byref(lens) if lens is not None else None, x, y, s0, n, _fptr(out)))
        return out
    if lens is not None:   # kyhip_kat_li_lens: the samples of a render under that lens (and pixel filter)
        _check(lib.kyhip_kat_li_lens(device, _scene_ptr(scene), C.byref(params), C.byref(filter) if filter is not None else None, C.byref(lens), x, y, s0, n, _fptr(out)))
        return out
    if filter is not None:   # kyhip_kat_li_filtered: the samples of a render under that pixel filter
        _check(lib.kyhip_kat_li_filtered(device, _scene_ptr(scene), C.byref(params), C.byref(filter), x, y, s0, n, _fptr(out)))
        return out
    _check(lib.kyhip_kat_li(device, _scene_ptr(scene), C.byref(params), x, y, s0, n, _fptr(out)))
    return out


def kat_li_lighting(scene, params, lighting, x, y, s0, n, device=0):
    """kyhip_kat_li_lighting: kat_li for the samples of render(..., lighting=lighting)."""
    lib = A.load_kyhip()
    out = np.zeros((n, 3), np.float32)
    _check(lib.kyhip_kat_li_lighting(device, _scene_ptr(scene), C.byref(params), int(lighting), x, y, s0, n, _fptr(out)))
    return out


def kat_nee(scene, direct_sample, light, in15, device=0):
    lib = A.load_kyhip()
    in15 = np.ascontiguousarray(in15, np.float32)
    out = np.zeros((in15.shape[0], 6), np.float32)
    _check(lib.kyhip_kat_nee(device, _scene_ptr(scene), direct_sample, light, _fptr(in15), in15.shape[0], _fptr(out)))
    return out


def kat_single_light(scene, in16, device=0):
    """kyhip_kat_single_light: rows of a kat_nee row + pick_u -> the picked light's two both_mis halves times the light count."""
    lib = A.load_kyhip()
    in16 = np.ascontiguousarray(in16, np.float32)
    out = np.zeros((in16.shape[0], 6), np.float32)
    _check(lib.kyhip_kat_single_light(device, _scene_ptr(scene), _fptr(in16), in16.shape[0], _fptr(out)))
    return out


def scene_light_pick(scene, rule=A.PICK_SPATIAL):
    """kyhip_scene_light_pick (host only): (the power rule's 16 probabilities, the emitter proxies [n, 11] = {light, kind, c[3], r, n[3], A, e}) that
    sample_single_light's power and spatial picks (direct_sample 113 / 177) read."""
    lib = A.load_kyhip()
    power = np.zeros(A.MAX_LIGHTS, np.float32)
    proxies = np.zeros((A.MAX_PROXIES, 11), np.float32)
    rc = lib.kyhip_scene_light_pick(_scene_ptr(scene), int(rule), _fptr(power), _fptr(proxies), A.MAX_PROXIES)
    if rc < 0:
        _check(rc)
    return power, proxies[:rc].copy()


def kat_light_pick(scene, rule, in16, device=0):
    """kyhip_kat_light_pick: kat_single_light's rows -> [n, 18] = {the picked light, its probability, every light's probability at the row's vertex}."""
    lib = A.load_kyhip()
    in16 = np.ascontiguousarray(in16, np.float32)
    out = np.zeros((in16.shape[0], 18), np.float32)
    _check(lib.kyhip_kat_light_pick(device, _scene_ptr(scene), int(rule), _fptr(in16), in16.shape[0], _fptr(out)))
    return out


def kat_single_light_rule(scene, rule, in16, device=0):
    """kyhip_kat_single_light_rule: kat_single_light with the light picked under `rule` (0 uniform, 1 power, 2 spatial), the halves over its probability."""
    lib = A.load_kyhip()
    in16 = np.ascontiguousarray(in16, np.float32)
    out = np.zeros((in16.shape[0], 6), np.float32)
    _check(lib.kyhip_kat_single_light_rule(device, _scene_ptr(scene), int(rule), _fptr(in16), in16.shape[0], _fptr(out)))
    return out


def kat_li_trace(scene, params, x, y, s, max_rows=64, device=0):
    """kyhip_kat_li_trace: (rows [n, 26], li [3]) of one camera sample of path_tracing_iteration_t."""
    lib = A.load_kyhip()
    rows = np.zeros((max_rows, 26), np.float32)
    li = np.zeros(3, np.float32)
    n = lib.kyhip_kat_li_trace(device, _scene_ptr(scene), C.byref(params), x, y, s, _fptr(rows), max_rows, _fptr(li))
    if n < 0:
        _check(n, lib)
    return rows[:n], li


def kat_sampler(seed, keys2, k, debug=False, device=0):
    """kyhip_kat_sampler: keys2 [n, 2] uint32 {pixel_index, sample_index} -> [n, k] uint32, the bit patterns of each stream's first k floats."""
    lib = A.load_kyhip()
    keys2 = np.ascontiguousarray(keys2, np.uint32)
    assert keys2.ndim == 2 and keys2.shape[1] == 2
    out = np.zeros((keys2.shape[0], k), np.uint32)
    _check(lib.kyhip_kat_sampler(device, int(seed) & 0xFFFFFFFF, keys2.ctypes.data_as(C.c_void_p), keys2.shape[0], k, int(bool(debug)),
                                 out.ctypes.data_as(C.c_void_p)), lib)
    return out


def kat_sampler_kind(kind, seed, spp, keys2, k, device=0, lib=None):
    """kyhip_kat_sampler_kind: kat_sampler for any sampler kind; spp is the frame's samples_per_pixel, which the stratified sampler's strata depend on."""
    lib = lib or A.load_kyhip()
    keys2 = np.ascontiguousarray(keys2, np.uint32)
    assert keys2.ndim == 2 and keys2.shape[1] == 2
    out = np.zeros((keys2.shape[0], k), np.uint32)
    _check(lib.kyhip_kat_sampler_kind(device, int(kind), int(seed) & 0xFFFFFFFF, int(spp), keys2.ctypes.data_as(C.c_void_p), keys2.shape[0], k,
                                      out.ctypes.data_as(C.c_void_p)), lib)
    return out


# ---- smallpt's own scene in double precision --------------------------------------

def smallpt_scene():
    """The 9 spheres of smallpt2pbrt/smallpt.cpp:42-52 as a ctypes array."""
    spheres = (A.SmallptSphere * 9)()
    n = A.load_kyhip().kyhip_smallpt_scene(spheres)
    assert n == 9
    return spheres


def smallpt_scene_rewrite():
    """Scene::CreateSmallptScene of smallpt2pbrt/smallpt_rewrite.cpp:1199-1244 (the same spheres at -z)."""
    spheres = (A.SmallptSphere * 9)()
    n = A.load_kyhip().kyhip_smallpt_scene_rewrite(spheres)
    assert n == 9
    return spheres


def smallpt_params(width, height, samps, seed=1234, max_depth=10, variant=A.SP_VARIANT_SMALLPT):
    return A.SmallptParams(width, height, samps, seed, max_depth, variant)


def smallpt_render(spheres, params, device=0):
    """kyhip_smallpt_render: smallpt's main() loop nest on the GPU; returns float64 [H, W, 3], row 0 = top of the picture."""
    lib = A.load_kyhip()
    img = np.zeros((params.height, params.width, 3), np.float64)
    _check(lib.kyhip_smallpt_render(device, spheres, len(spheres), C.byref(params), img.ctypes.data_as(C.c_void_p)), lib)
    return img


def smallpt_kat_radiance(spheres, params, x, y, sx, sy, s0, n, device=0):
    lib = A.load_kyhip()
    out = np.zeros((n, 3), np.float64)
    _check(lib.kyhip_smallpt_kat_radiance(device, spheres, len(spheres), C.byref(params), x, y, sx, sy, s0, n,
                                          out.ctypes.data_as(C.c_void_p)), lib)
    return out


def smallpt_kat_rng(seed, keys2, k, device=0):
    """kyhip_smallpt_kat_rng: keys2 [n, 2] uint32 {subpixel_index, sample} -> [n, k] uint64, the bit patterns of each stream's first k doubles."""
    lib = A.load_kyhip()
    keys2 = np.ascontiguousarray(keys2, np.uint32)
    assert keys2.ndim == 2 and keys2.shape[1] == 2
    out = np.zeros((keys2.shape[0], k), np.uint64)
    _check(lib.kyhip_smallpt_kat_rng(device, int(seed) & 0xFFFFFFFF, keys2.ctypes.data_as(C.c_void_p), keys2.shape[0], k,
                                     out.ctypes.data_as(C.c_void_p)), lib)
    return out


def store_image(filename, rgb, kind="bmp"):
    """film_t::store_{ppm,bmp,hdr}_impl -- ky.cpp:1646-1782."""
    host = A.load_kyhost()
    rgb = np.ascontiguousarray(rgb, np.float32)
    k = {"ppm": 0, "bmp": 1, "hdr": 2}[kind]
    if host.kyhost_store_image(filename.encode(), k, rgb.shape[1], rgb.shape[0], _fptr(rgb)) != 0:
        raise KyError("store_image failed: " + host.kyhost_last_error().decode())
