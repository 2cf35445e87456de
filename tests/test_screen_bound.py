"""CPU: the live rectangle of a packed scene (kyhip_scene_screen_bound; ky_pack.cpp, screen_bound) -- the pixel rectangle outside which no camera ray reaches a
surface, so that the render kernels skip the 8 x 8 blocks outside it.  Its geometry on the Cornell box, its soundness against the oracle (every pixel outside
it is exactly 0 in the oracle's film), the cases in which it must be the whole frame, and the switch."""
import ctypes as C

import numpy as np
import pytest

from helpers import CustomScene, make_light, make_material, make_shape
from screen_cull_scenes import cornell_with_camera, inside_camera, moved_cameras


def bound(api, scene, w, h, **kw):
    return api.scene_screen_bound(scene, api.make_params(w, h, 4, **kw))


def test_cornell_geometry(A, api):
    """create_cornell_box_scene's 4 : 3 frame: the box covers the middle columns only (its opening subtends 0.446 of front, the frame's half-width is 0.559)."""
    (x0, y0, x1, y1), dead, total = bound(api, api.cornell_box_scene(A.CB_DEFAULT_SCENE, 1024, 768), 1024, 768)
    print("1024 x 768:", (x0, y0, x1, y1), dead, total)
    assert (y0, y1) == (0, 768) and 0 < x0 < x1 < 1024          # every row, not every column
    assert total == 12288 and dead >= 0.16 * total
    assert dead == ((x0 // 8) + (1024 - x1) // 8) * 96           # whole 8-pixel columns left and right of it
    for w, h in ((1024, 1024), (64, 48)):
        rect, dead, total = bound(api, api.cornell_box_scene(A.CB_DEFAULT_SCENE, w, h), w, h)
        print(w, "x", h, ":", rect, dead, total)
        assert dead == 0 and total == (w // 8) * (h // 8)
    rect, dead, total = bound(api, api.cornell_box_scene(A.CB_DEFAULT_SCENE, 256, 192), 256, 192)
    print("256 x 192:", rect, dead, total)
    assert total == 768 and 96 <= dead <= 128


def test_counts_follow_the_tiling(A, api):
    """dead / total are those of the shard the parameters name: the shards of a tiling share the frame's dead blocks among them, ragged tiles included"""
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 100, 75)
    rect, dead, total = bound(api, scene, 100, 75, tile_w=16, tile_h=16)
    assert total == 7 * 5 * 4 and dead > 0
    parts = [bound(api, scene, 100, 75, tile_w=16, tile_h=16, tile_first=r, tile_step=3) for r in range(3)]
    assert all(p[0] == rect for p in parts)
    assert sum(p[1] for p in parts) == dead and sum(p[2] for p in parts) == total
    other = bound(api, scene, 100, 75, tile_w=32, tile_h=8)
    assert other[0] == rect and other[2] == 4 * 10 * 4


def test_a_distant_sphere_gets_a_small_rectangle(A, api):
    """One unit sphere 20 units in front of a camera: the rectangle is at most four times the sphere's own projected box (not trivially the whole frame)."""
    W = H = 256
    t = 0.5                                                      # tan(fov / 2): the frame is one unit wide at unit depth
    cam = A.Camera()
    for j, (p, f, r, u) in enumerate(zip((0, 0, 0), (0, 0, 1), (t, 0, 0), (0, t, 0))):
        cam.position[j], cam.front[j], cam.right[j], cam.up[j] = p, f, r, u
    cam.resolution[0], cam.resolution[1] = W, H
    scene = CustomScene(A, cam, [make_shape(A, A.SHAPE_SPHERE, [(0, 0, 20)], radius=1.0)], [make_material(A, A.MATERIAL_MATTE, (0.5, 0.5, 0.5))],
                        [make_light(A, A.LIGHT_POINT, (1, 1, 1), position=(0, 5, 0))], [A.Surface(0, 0, -1)])
    (x0, y0, x1, y1), dead, total = bound(api, scene, W, H)
    half = (1.0 / np.sqrt(20.0 ** 2 - 1.0)) / t * W              # the silhouette's tangent rays: tan(asin(r / d)), in pixels
    print("sphere:", (x0, y0, x1, y1), "projected box", 2 * half)
    assert x0 <= W / 2 - half and x1 >= W / 2 + half and y0 <= H / 2 - half and y1 >= H / 2 + half
    assert (x1 - x0) * (y1 - y0) <= 4 * (2 * half) ** 2
    assert dead > 0.8 * total


@pytest.fixture(scope="module")
def cameras(A, api):
    return moved_cameras(A, api, 128, 96)


def _outside_is_black(api, O, scene, w, h):
    """the oracle's film at 4 spp over the whole frame: exactly 0 outside the rectangle; -> (rectangle, pixels outside, lit pixels inside)"""
    p = api.make_params(w, h, 4)
    (x0, y0, x1, y1), _, _ = api.scene_screen_bound(scene, p)
    film = O.render(scene, p)
    outside = np.ones((h, w), bool)
    outside[y0:y1, x0:x1] = False
    assert not film[outside].any(), (x0, y0, x1, y1)
    return (x0, y0, x1, y1), int(outside.sum()), int((film[~outside].max(axis=-1) > 0).sum()) if (~outside).any() else 0


def test_outside_is_black_in_the_oracle_cornell(A, api, O):
    rect, n_out, lit = _outside_is_black(api, O, api.cornell_box_scene(A.CB_DEFAULT_SCENE, 256, 192), 256, 192)
    print("cornell 256 x 192:", rect, n_out, lit)
    assert n_out >= 96 * 64 and lit > 0.5 * (256 * 192 - n_out)


def test_outside_is_black_in_the_oracle_moved_cameras(A, api, O, cameras):
    W, H = 128, 96
    seen = {}
    for name, scene in cameras.items():
        seen[name] = _outside_is_black(api, O, scene, W, H)
        print(name, seen[name])
    (x0, y0, x1, y1), n_out, lit = seen["back"]
    assert 0 < x0 < x1 < W and 0 < y0 < y1 < H and lit > 0       # the whole bound inside the frame
    for name in ("right", "up"):                                 # the bound partly off-screen: the rectangle ends at a frame edge, and is not the whole frame
        (x0, y0, x1, y1), n_out, lit = seen[name]
        assert (x0 == 0 or x1 == W or y0 == 0 or y1 == H) and n_out > 0 and lit > 0, name
    assert seen["roll"][1] > 0 and seen["roll"][2] > 0
    (x0, y0, x1, y1), n_out, lit = seen["away"]                  # the box behind the camera: nothing is live
    assert (x1 - x0) * (y1 - y0) == 0 and n_out == W * H


def test_refusals(A, api):
    """the whole frame where the proof does not hold"""
    W, H = 256, 192
    env = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_ENVIRONMENT, W, H)
    assert bound(api, env, W, H) == ((0, 0, W, H), 0, 768)
    both = api.cornell_box_scene(A.CB_DEFAULT_SCENE | A.CB_LIGHT_ENVIRONMENT, W, H)
    assert bound(api, both, W, H) == ((0, 0, W, H), 0, 768)
    assert bound(api, inside_camera(A, api, W, H), W, H) == ((0, 0, W, H), 0, 768)
    nan = cornell_with_camera(A, api, W, H, lambda cam: A.Camera.from_buffer_copy(cam))
    nan.shapes[0].p[2][1] = float("nan")
    assert bound(api, nan, W, H) == ((0, 0, W, H), 0, 768)


def test_the_switch(A, api):
    lib = A.load_kyhip()
    W, H = 256, 192
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H)
    on = bound(api, scene, W, H)
    assert on[1] > 0
    assert lib.kyhip_set_screen_cull(-1) == 1 and lib.kyhip_set_screen_cull(-1) == 1   # a query changes nothing
    prev = lib.kyhip_set_screen_cull(0)
    try:
        assert prev == 1 and lib.kyhip_set_screen_cull(-1) == 0
        assert bound(api, scene, W, H) == ((0, 0, W, H), 0, 768)
    finally:
        lib.kyhip_set_screen_cull(prev)
    assert bound(api, scene, W, H) == on


def test_bad_arguments(A, api):
    lib = A.load_kyhip()
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 64, 48)
    rect = (C.c_int * 4)()
    assert lib.kyhip_scene_screen_bound(scene.flat, C.byref(api.make_params(64, 48, 4, tile_w=12)), rect, None) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_scene_screen_bound(scene.flat, C.byref(api.make_params(64, 48, 4)), None, None) == A.KY_ERR_INVALID_VALUE
    assert lib.kyhip_scene_screen_bound(scene.flat, C.byref(api.make_params(64, 48, 4)), rect, None) == A.KY_OK
    assert 0 < rect[0] < 8 and 56 < rect[2] < 64 and (rect[1], rect[3]) == (0, 48)   # narrower than the frame, by less than a block on either side
