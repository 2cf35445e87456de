"""Temporal reuse in a frame's denoise filter, on the GPU (include/kyhip.h, kyhip_history_* and kyhip_frame_denoise_temporal; DESIGN.md "Denoise", "Temporal"):
denoise_temporal_kernel (ky_amd/csrc/ky_denoise.hip) and the levels behind it against the NumPy restatement of tests/denoise_temporal_restatement.py, fed each
frame's own checkpoint, guides, keys and albedo along a short camera path; what an empty history, a reset and two identical sequences return; that the kernel finds
surfaces again, leaves uncovered ones alone and keeps its hands off what mirrors and glass show; and the claim: temporal + spatial lies below spatial alone."""
import ctypes as C

import numpy as np
import pytest

import denoise_albedo_restatement as DA
import denoise_restatement as D
import denoise_temporal_restatement as DT
import noise_restatement as R
import test_denoise_gpu as T
import texture_restatement as X
from screen_cull_scenes import cornell_with_camera

pytestmark = pytest.mark.gpu

W, H = 40, 24


def _scene_at(A, api, w, h, s, textured=False, tilt=0.0):
    """The denoise tests' Cornell scene (textured: tests/texture_restatement.py's cornell_case) seen from the fraction s of DT's camera path
    -> (scene, the restatement's textures, the frame's textures)"""
    if textured:
        scene, textures = X.cornell_case(A, api, w, h)
        scene.scene.camera = DT.path_camera(A, scene.scene.camera, s, tilt)
        return scene, textures, [t.to_api(api) for t in textures]
    return cornell_with_camera(A, api, w, h, lambda cam: DT.path_camera(A, cam, s, tilt)), [], None


def _gathered(f, w, h, total, **tile):
    """(the gather's cv in film order, the samples the frame holds) from the frame's own checkpoint"""
    n_pix = T._n_pix(w, h, **tile)
    done, accum, flags, (nb, n_prev, y_prev, m2) = R.split_state(f.save(), n_pix)
    return T._to_film(D.gather(accum, flags, m2, total, done, nb), w, h, **tile), done


def _within(got, want, ulps):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = float((err / np.maximum(np.abs(want.astype(np.float64)), 1e-300)).max())
    return bool((err <= ulps * 2.0 ** -23 * np.abs(want.astype(np.float64))).all()), rel


KERNEL_CASES = [("plain", 40, 24, 16, 16, 0, 0), ("plain", 44, 21, 16, 16, 1, 0), ("plain", 44, 21, 8, 24, 0, 0), ("plain", 264, 40, 16, 16, 1, 0),
                ("textured", 40, 24, 16, 16, 0, 2), ("textured", 44, 21, 8, 24, 1, 2), ("textured", 40, 24, 16, 16, 1, 0), ("textured", 44, 21, 16, 16, 0, 0)]


@pytest.mark.parametrize("which,w,h,tile_w,tile_h,bounces,grid", KERNEL_CASES, ids=["%s_%dx%d_tile_%dx%d_bounces_%d_albedo_%d" % c for c in KERNEL_CASES])
def test_kernels_against_the_restatement(which, w, h, tile_w, tile_h, bounces, grid, A, api):
    """Three frames along a dolly-and-pan path (s = 0, 0.5, 1 of DT's), the random sampler, 48 samples in passes of 8, 24 and 16, one history.  After every call
    History.read() meets the CPU test's bound for the step alone (rtol 2 x 2^-23, atol 0) and the film its bound through the levels ((levels + 2) x 2^-23);
    pass-through pixels to the bit.  264 x 40: wider than a workgroup, wavefronts straddle rows.  The restatement carries its OWN history from call to call.
    Measured on the MI355X: the largest relative difference of the history's colour / variance, of its counts and of the film is 0 in all eight cases (printed);
    DESIGN.md "Temporal"."""
    tile = dict(tile_w=tile_w, tile_h=tile_h)
    params = dict(D.DEFAULTS)
    restated = DT.History()
    worst = [0.0, 0.0, 0.0]
    with api.History(w, h) as hist:
        assert hist.frames == 0 and hist.ms() < 0 and not hist.read()[0].any() and not hist.read()[1].any()
        for k, s in enumerate((0.0, 0.5, 1.0)):
            scene, textures, tx = _scene_at(A, api, w, h, s, which == "textured")
            with api.Frame(scene, api.make_params(w, h, 48, seed=1234 + k, **tile), noise=True, textures=tx, guide_bounces=bounces, albedo=grid) as f:
                for n in (8, 24, 16):
                    f.render(n)
                assert f.done == 48
                got = f.denoise(params, history=hist)
                cv, done = _gathered(f, w, h, 48, **tile)
                ga, gb = f.guides()
                key = f.guide_chains() if bounces > 0 else None
                albedo = f.albedo() if grid > 0 else None
                if grid > 0:
                    cv = DA.demodulate(cv, gb, albedo)
                want = restated.step(cv, ga, gb, key, scene.scene.camera, w, done, params, albedo=albedo)
            assert hist.frames == k + 1 == restated.frames and hist.ms() > 0
            got_cv, got_m = hist.read()
            want_cv, want_m = restated.read()
            surface = gb[..., 3] == D.SURFACE
            eligible = surface if key is None else surface & (key == 0)
            assert np.array_equal(got_cv[~eligible], cv[~eligible]) and (got_m[~eligible] == 0).all()
            assert (got_m[eligible & ~restated.took] == done).all() and np.array_equal(got_cv[~restated.took], cv[~restated.took])
            if k > 0:
                assert restated.took.sum() > 0.3 * eligible.sum(), (int(restated.took.sum()), int(eligible.sum()))   # (pixels that find none: test_it_finds_the_surfaces_again)
            oks = [_within(got_cv, want_cv, 2), _within(got_m, want_m, 2), _within(got, np.clip(want[..., :3], 0.0, 1.0), params["levels"] + 2)]
            worst = [max(a, b[1]) for a, b in zip(worst, oks)]
            assert all(ok for ok, _ in oks), (k, [rel for _, rel in oks])
    print("largest relative |GPU - restatement| (%s %d x %d, tile %d x %d, %d bounces, albedo %d): history colour / variance %.3e, count %.3e, film %.3e" % (
        which, w, h, tile_w, tile_h, bounces, grid, worst[0], worst[1], worst[2]))


def _three(api, scenes, hist, **kw):
    """One sequence: a frame of 48 samples per scene, each denoised into `hist` -> the films"""
    films = []
    for k, scene in enumerate(scenes):
        with api.Frame(scene, api.make_params(W, H, 48, seed=77 + k), noise=True, guide_bounces=1) as f:
            f.render(24)
            f.render(24)
            films.append(f.denoise(history=hist, **kw))
    return films


def test_empty_history_reset_and_determinism(A, api):
    """With a fresh history the film equals Frame.denoise()'s bit for bit and the history holds the gather's cv with m = the pixel's samples; reset() restores
    that state; two identical sequences return identical bytes; levels = 0 delivers the accumulated picture, clamped, unfiltered"""
    scenes = [_scene_at(A, api, W, H, s)[0] for s in (0.0, 0.5, 1.0)]
    with api.History(W, H) as hist, api.History(W, H) as other:
        with api.Frame(scenes[0], api.make_params(W, H, 48, seed=77), noise=True, guide_bounces=1) as f:
            f.render(24)
            f.render(24)
            before = f.save()
            plain = f.denoise()
            first = f.denoise(history=hist)
            assert first.tobytes() == plain.tobytes() and f.save() == before and hist.frames == 1
            cv, done = _gathered(f, W, H, 48)
            ga, gb = f.guides()
            key = f.guide_chains()
            got_cv, got_m = hist.read()
            eligible = (gb[..., 3] == D.SURFACE) & (key == 0)
            assert got_cv.tobytes() == cv.tobytes() and np.array_equal(got_m, np.where(eligible, np.float32(done), np.float32(0)))
            again = f.denoise(history=hist)                   # the same frame against its own history: counted twice, and no longer the plain film
            assert hist.frames == 2 and (hist.read()[1][eligible] == 2 * done).mean() > 0.9 and not np.array_equal(again, plain)
            hist.reset()
            assert hist.frames == 0 and not hist.read()[1].any() and hist.ms() > 0
            assert f.denoise(history=hist).tobytes() == plain.tobytes() and hist.read()[0].tobytes() == cv.tobytes()
            hist.reset()
        a, b = _three(api, scenes, hist), _three(api, scenes, other)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert hist.read()[0].tobytes() == other.read()[0].tobytes() and hist.read()[1].tobytes() == other.read()[1].tobytes()
        with api.Frame(scenes[2], api.make_params(W, H, 48, seed=79), noise=True, guide_bounces=1) as f:
            f.render(24)
            f.render(24)
            plain = f.denoise()
            assert not np.array_equal(a[2], plain)            # the history is seen
            unfiltered = f.denoise(dict(levels=0), history=hist)
            assert np.array_equal(unfiltered, np.clip(hist.read()[0][..., :3], 0.0, 1.0))


def test_it_finds_the_surfaces_again(A, api):
    """80 x 48, guide bounces 1, the camera moved along the whole path between two frames.  On the host, from the two frames' guides and keys: a class-0, key-0
    pixel of the second frame whose reprojection's four taps all lie on the first frame's mirror or glass ball (key != 0) was hidden behind that ball -- it reads
    m = n_p and keeps the gather's bits.  A back-wall pixel (its normal against the viewing direction) whose four taps are back-wall pixels of the first frame
    reads m > n_p.  The balls' own pixels (key != 0) read m = 0 in both frames."""
    w, h = 80, 48
    guides = []
    with api.History(w, h) as hist:
        for k, s in enumerate((0.0, 1.0)):
            scene = _scene_at(A, api, w, h, s)[0]
            with api.Frame(scene, api.make_params(w, h, 32, seed=5 + k), noise=True, guide_bounces=1) as f:
                f.render(16)
                f.render(16)
                f.denoise(history=hist)
                cv, done = _gathered(f, w, h, 32)
                ga, gb = f.guides()
                guides.append((ga, gb, f.guide_chains(), scene.scene.camera, cv, done))
            got_cv, m = hist.read()
            key = guides[-1][2]
            assert (key != 0).sum() > 40 and (m[key != 0] == 0).all() and (m[(gb[..., 3] == D.SURFACE) & (key == 0)] >= done).all()
    (ga1, gb1, key1, cam1, _, _), (ga2, gb2, key2, cam2, cv2, n_p) = guides
    sx, sy, z = DT.project(gb2[..., :3], DT.camera_vectors(cam1), w, h)
    eligible = (gb2[..., 3] == D.SURFACE) & (key2 == 0)
    inside = eligible & (z > 0) & (sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1)
    i0, j0 = np.floor(np.where(inside, sx, 0)).astype(int), np.floor(np.where(inside, sy, 0)).astype(int)
    taps = lambda a: np.stack([a[j0 + dj, i0 + di] for dj in (0, 1) for di in (0, 1)])
    uncovered = inside & (taps(key1) != 0).all(axis=0)
    f1, f2 = DT.camera_vectors(cam1)[1], DT.camera_vectors(cam2)[1]
    back1 = (gb1[..., 3] == D.SURFACE) & (key1 == 0) & (ga1[..., :3].astype(np.float64) @ f1 < -0.99)
    back2 = inside & (ga2[..., :3].astype(np.float64) @ f2 < -0.98)
    found = back2 & taps(back1).all(axis=0)
    print("80 x 48: %d pixels uncovered behind a ball, %d back-wall pixels found again; m there %.1f .. %.1f" % (
        int(uncovered.sum()), int(found.sum()), m[found].min(), m[found].max()))
    assert uncovered.sum() >= 4 and found.sum() >= 200
    assert (m[uncovered] == n_p).all() and np.array_equal(got_cv[uncovered], cv2[uncovered])
    assert (m[found] > n_p).all()


_truth = {}


def _path_truth(A, api, tilt):
    """api.render at 16 384 samples of the path's last frame, and the pixels further than 2 pixels from a saturated one of it (a channel >= 0.9), once per
    path.  Never modified."""
    if tilt not in _truth:
        film = api.render(_scene_at(A, api, W, H, 1.0, tilt=tilt)[0], api.make_params(W, H, 16384, seed=987654))
        film.setflags(write=False)
        bright = film.max(axis=2) >= 0.9
        near = np.zeros_like(bright)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                near |= bright[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]
        _truth[tilt] = (film, ~near)
    return _truth[tilt]


@pytest.mark.parametrize("seed", [DT.PATH_SEED, 101, 202])
@pytest.mark.parametrize("path", ["lamp_out_of_view", "lamp_in_view"])
def test_it_denoises(path, seed, A, api):
    """The CPU replay's paths (tools/denoise_replay.py temporal; profiles/denoise_temporal_replay.txt): DT.PATH_FRAMES frames of DT.PATH_SPP samples in passes of
    4 along DT's camera path, frame k with seed + k, guide bounces 1, the defaults; the truth is api.render at 16 384 samples of the last frame.
    lamp_out_of_view (every frame tilted down by DT.PATH_TILT): the WHOLE-FILM RMSE of temporal + spatial lies BELOW that of spatial alone (the same frame's
    denoise()).  The condition is "below"; the replay gave 0.87 .. 0.94, the MI355X 0.870 0.941 0.920 (seeds 1234, 101, 202).
    lamp_in_view: the replay's whole-film ratio is NOT below 1 there (1.26 .. 1.93), and not because of the floor's highlight: a pixel that the lamp covers in
    part has a class-0 centre ray and an unclamped mean of several times white, and the temporal step -- which has no luminance term and no colour clamp -- blends
    it with history that saw ceiling, and the ceiling beside it with history that saw lamp.  Over the pixels the replay names, those further than 2 pixels from a
    saturated pixel of the truth, the ratio is 0.60 .. 0.80: that is the condition here, and the whole-film figure is printed.  DESIGN.md "Temporal" says so.
    Measured on the MI355X: whole film 1.257 1.352 1.925, away from saturated pixels 0.803 0.606 0.602."""
    tilt = DT.PATH_TILT if path == "lamp_out_of_view" else 0.0
    truth, away = _path_truth(A, api, tilt)
    truth = truth.astype(np.float64)
    rmse = lambda film, sel: float(np.sqrt((((film.astype(np.float64) - truth) ** 2)[sel]).mean()))
    with api.History(W, H) as hist:
        for k in range(DT.PATH_FRAMES):
            scene = _scene_at(A, api, W, H, k / (DT.PATH_FRAMES - 1), tilt=tilt)[0]
            with api.Frame(scene, api.make_params(W, H, DT.PATH_SPP, seed=seed + k), noise=True, guide_bounces=1) as f:
                while f.render(1) < f.total:
                    pass
                both = f.denoise(history=hist)
                spatial, raw = f.denoise(), f.resolve(normalise=True)
    everywhere = np.ones((H, W), bool)
    e, a = [rmse(x, everywhere) for x in (raw, spatial, both)], [rmse(x, away) for x in (raw, spatial, both)]
    print("%s, seed %d, frame %d at %d samples: whole film RMSE raw %.5f spatial %.5f temporal + spatial %.5f: / spatial %.3f; %d pixels away from saturated ones: "
          "%.5f %.5f %.5f: / spatial %.3f" % (path, seed, DT.PATH_FRAMES, DT.PATH_SPP, e[0], e[1], e[2], e[2] / e[1], int(away.sum()), a[0], a[1], a[2], a[2] / a[1]))
    if path == "lamp_out_of_view":
        assert e[2] < e[1], e
    else:
        assert away.sum() > 0.85 * W * H and a[2] < a[1], a


def test_shapes_of_use(A, api, O):
    """One history used by a frame under a tent filter and then by one under a lens (the guides stay pinhole); a pinned film added to in place and a pageable
    one agree to the bit; a sub-film's origin and row stride"""
    import test_lens_gpu as TL
    scenes = [_scene_at(A, api, W, H, s)[0] for s in (0.0, 0.5)]
    lens = TL.lens_of(O, A, api, "cornell", W, H)[0]
    forms = (dict(filter=api.pixel_filter(A.FILTER_TENT, 2.0)), dict(lens=lens))

    def sequence(hist, deliver):
        out = []
        for k, (scene, kw) in enumerate(zip(scenes, forms)):
            with api.Frame(scene, api.make_params(W, H, 48, seed=9 + k), noise=True, guide_bounces=1, **kw) as f:
                f.render(24)
                f.render(24)
                out.append(deliver(f, hist))
        return out

    with api.History(W, H) as h1, api.History(W, H) as h2, api.History(W, H) as h3:
        pageable = sequence(h1, lambda f, hist: f.denoise(history=hist))
        assert all(np.isfinite(x).all() for x in pageable) and (h1.read()[1] > 48).sum() > 300      # the lens frame found the tent frame's surfaces
        pinned = api.PinnedFilm(H, W)

        def in_place(f, hist):
            pinned.array[:] = 0
            assert f.denoise(film=pinned.array, history=hist) is pinned.array
            return pinned.array.copy()

        assert all(np.array_equal(x, y) for x, y in zip(sequence(h2, in_place), pageable))

        def sub_film(f, hist):
            big = np.full((H + 5, W + 9, 3), 0.25, np.float32)
            f.denoise(film=big, origin_px=(4, 3), history=hist)
            out = big[3:3 + H, 4:4 + W] - np.float32(0.25)
            big[3:3 + H, 4:4 + W] = 0.25
            assert (big == 0.25).all()
            return big, out

        for (big, out), want in zip(sequence(h3, sub_film), pageable):
            assert np.array_equal(out + np.float32(0.25), want + np.float32(0.25))
        assert h1.read()[0].tobytes() == h2.read()[0].tobytes() == h3.read()[0].tobytes()


def test_refusals(A, api):
    """With a frame and a device: each refusal leaves the film, the history and the next call what they were"""
    lib = A.load_kyhip()
    scene, textures, tx = _scene_at(A, api, W, H, 0.0, textured=True)
    p = api.make_params(W, H, 48)
    film = np.full((H, W, 3), 7.0, np.float32)
    ptr = C.c_void_p(film.ctypes.data)
    with api.History(W, H) as hist, api.History(W + 4, H) as wide, api.History(W, H - 3) as low:
        with api.Frame(scene, p, noise=True, textures=tx) as f:
            f.render(24)
            with pytest.raises(api.KyError, match="noise batches"):
                f.denoise(history=hist)
            f.render(24)
            assert lib.kyhip_frame_denoise_temporal(f._f, None, None, None, ptr, W) == A.KY_ERR_INVALID_VALUE and b"history is NULL" in lib.kyhip_last_error()
            assert lib.kyhip_frame_denoise_temporal(f._f, hist._h, None, None, None, W) == A.KY_ERR_INVALID_VALUE and b"film" in lib.kyhip_last_error()
            assert lib.kyhip_frame_denoise_temporal(f._f, hist._h, None, None, ptr, W - 1) == A.KY_ERR_INVALID_VALUE and b"film" in lib.kyhip_last_error()
            for other, word in ((wide, "the history is 44 x 24"), (low, "the history is 40 x 21")):
                with pytest.raises(api.KyError, match=word):
                    f.denoise(history=other)
            with pytest.raises(api.KyError, match="max_history"):
                f.denoise(history=hist, temporal=dict(max_history=0.0))
            with pytest.raises(api.KyError, match="levels"):
                f.denoise(dict(levels=7), history=hist)
            with pytest.raises(ValueError):
                f.denoise(temporal=dict(max_history=2.0))
            assert (film == 7).all() and hist.frames == 0 and wide.frames == 0 and hist.ms() < 0
            plain = f.denoise()
            assert np.array_equal(f.denoise(history=hist), plain) and hist.frames == 1
        with api.Frame(scene, p, noise=True, textures=tx, albedo=2) as f:     # the history holds plain colours
            f.render(24)
            f.render(24)
            with pytest.raises(api.KyError, match="plain colours"):
                f.denoise(history=hist)
            assert hist.frames == 1
            hist.reset()
            f.denoise(history=hist)
        with api.Frame(scene, p, noise=True, textures=tx) as f:               # ... and now demodulated ones
            f.render(24)
            f.render(24)
            with pytest.raises(api.KyError, match="albedo-demodulated"):
                f.denoise(history=hist)
            assert hist.frames == 1
        hist.reset()
        with api.Frame(scene, p, noise=True, blocks=True, textures=tx) as f:
            f.render(24)
            f.render(24)
            with pytest.raises(api.KyError, match="tracks blocks"):
                f.denoise(history=hist)
        with api.Frame(scene, api.make_params(W, H, 48, tile_first=0, tile_step=2), noise=True, textures=tx) as f:
            f.render(24)
            f.render(24)
            with pytest.raises(api.KyError, match="shard"):
                f.denoise(history=hist)
        with api.Frame(scene, p, textures=tx) as f:
            f.render(24)
            with pytest.raises(api.KyError, match="kyhip error -1"):
                f.denoise(history=hist)
        assert hist.frames == 0
