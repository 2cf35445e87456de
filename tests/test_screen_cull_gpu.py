"""GPU: the screen cull (kyhip_set_screen_cull; ky_render.hpp's work decoder skips the 8 x 8 blocks outside the scene's live rectangle) changes no bit of a film.
Every kernel family the decoder serves renders the Cornell box with the switch on and off at 96 x 72 -- the smallest 4 : 3 frame with dead blocks, block 0 among
them -- and at 100 x 75 (ragged tiles): np.array_equal.  Then a frame in which EVERY block is dead, and one under an environment light, where nothing is."""
import numpy as np
import pytest

from screen_cull_scenes import moved_cameras

pytestmark = pytest.mark.gpu
SPP, DEPTH = 64, 5
SIZES = [(96, 72), (100, 75)]


@pytest.fixture(scope="module")
def lib(A):
    lib = A.load_kyhip()
    prev = lib.kyhip_set_jit(0)
    yield lib
    lib.kyhip_set_jit(prev)


def on_and_off(lib, render):
    """render() with the cull on, then off"""
    prev = lib.kyhip_set_screen_cull(1)
    try:
        on = render()
        lib.kyhip_set_screen_cull(0)
        off = render()
    finally:
        lib.kyhip_set_screen_cull(prev)
    return on, off


def frame_in_passes(api, scene, p, **kw):
    with api.Frame(scene, p, **kw) as f:
        while f.render(p.samples_per_pixel // 3) < p.samples_per_pixel:
            pass
        return f.resolve()


def _hot(A, api, lib, scene, w, h):
    film = api.render(scene, api.make_params(w, h, SPP, max_path_depth=DEPTH))
    assert b"strategy 48, feat 3975" in lib.kyhip_last_kernel(0), lib.kyhip_last_kernel(0)   # the headline row
    return film


def _masked(A, api, lib, scene, w, h):
    film = api.render(scene, api.make_params(w, h, SPP, max_path_depth=DEPTH), lighting=A.LIGHTING_DIRECT | A.LIGHTING_INDIRECT)
    assert b"drop 1" in lib.kyhip_last_kernel(0), lib.kyhip_last_kernel(0)
    return film


def _run_time_dispatched(A, api, lib, scene, w, h):
    prev = lib.kyhip_set_specialisation(0)
    try:
        film = api.render(scene, api.make_params(w, h, SPP, max_path_depth=DEPTH, direct_sample=A.DIRECT_LIGHT_MIS))
        assert b"strategy -1" in lib.kyhip_last_kernel(0), lib.kyhip_last_kernel(0)   # strategy and integrator read from the launch constants
    finally:
        lib.kyhip_set_specialisation(prev)
    return film


def _normal_aov(A, api, lib, scene, w, h):
    return api.render(scene, api.make_params(w, h, SPP, max_path_depth=DEPTH, integrator=A.INTEGRATOR_NORMAL, sampler=A.SAMPLER_DEBUG))


def _single_light(A, api, lib, scene, w, h):
    return api.render(scene, api.make_params(w, h, SPP, max_path_depth=DEPTH, direct_sample=A.DIRECT_SINGLE_BOTH_MIS))


def _shard(A, api, lib, scene, w, h):
    return api.render(scene, api.make_params(w, h, SPP, max_path_depth=DEPTH, tile_first=1, tile_step=2))


def _three_passes(A, api, lib, scene, w, h):
    return frame_in_passes(api, scene, api.make_params(w, h, SPP, max_path_depth=DEPTH))


def _block_tracking(A, api, lib, scene, w, h):
    return frame_in_passes(api, scene, api.make_params(w, h, SPP, max_path_depth=DEPTH), blocks=True)


FAMILIES = {"hot": _hot, "masked": _masked, "run_time_dispatched": _run_time_dispatched, "normal_aov": _normal_aov, "single_light": _single_light, "shard": _shard,
            "three_passes": _three_passes, "block_tracking": _block_tracking}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_cull_changes_no_bit(family, size, A, api, lib):
    w, h = size
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h)
    rect, dead, total = api.scene_screen_bound(scene, api.make_params(w, h, SPP))
    assert dead >= 9 and rect[0] >= 8, (rect, dead, total)        # block 0 (the frame's corner) is dead: some wavefront's own item is skipped
    on, off = on_and_off(lib, lambda: FAMILIES[family](A, api, lib, scene, w, h))
    assert np.array_equal(on, off)
    assert on.max() > 0 and not on[:, :rect[0]].any() and not on[:, rect[2]:].any()


def test_everything_dead(A, api, lib):
    """A camera that looks away from the box: every block is dead -- every wavefront's own item, and there are fewer items than wavefronts.  The launch ends; the film is black."""
    w, h = 96, 72
    scene = moved_cameras(A, api, w, h)["away"]
    p = api.make_params(w, h, SPP, max_path_depth=DEPTH)
    rect, dead, total = api.scene_screen_bound(scene, p)
    assert dead == total == 6 * 5 * 4        # every block of the 6 x 5 tiles of 16 x 16 pixels (the last tile row is half outside the frame)
    on, off = on_and_off(lib, lambda: api.render(scene, p))
    assert not on.any() and not off.any()
    assert not frame_in_passes(api, scene, p, blocks=True).any()


def test_environment_light_is_not_culled(A, api, lib):
    """Under the environment light a miss adds radiance: the bands beside the box are lit, nothing is dead, and the switch changes nothing."""
    w, h = 96, 72
    rect, dead, _ = api.scene_screen_bound(api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h), api.make_params(w, h, SPP))
    scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_ENVIRONMENT, w, h)
    p = api.make_params(w, h, SPP, max_path_depth=DEPTH)
    assert api.scene_screen_bound(scene, p)[1] == 0 and dead > 0
    on, off = on_and_off(lib, lambda: api.render(scene, p))
    assert np.array_equal(on, off)
    assert (on[:, :rect[0]].max(axis=-1) > 0).all() and (on[:, rect[2]:].max(axis=-1) > 0).all()
