"""Scenes of the screen-cull tests (kyhip_scene_screen_bound, kyhip_set_screen_cull): the Cornell box seen by cameras that are moved and turned, shared by the
CPU tests (tests/test_screen_bound.py) and the GPU tests (tests/test_screen_cull_gpu.py)."""
import numpy as np

from helpers import CustomScene

SEED = 20260117


def _unit(v):
    return v / np.linalg.norm(v)


def camera_like(A, cam, position, front, up_hint):
    """camera_t's constructor (ky.cpp:1875-1879) with another position and viewing direction: the field of view and the aspect ratio of `cam` are kept."""
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    tan_fov = np.linalg.norm(f32(cam.up))
    aspect = np.linalg.norm(f32(cam.right)) / tan_fov
    front = _unit(np.asarray(front, np.float64))
    right = _unit(np.cross(np.asarray(up_hint, np.float64), front)) * tan_fov * aspect
    up = _unit(np.cross(front, right)) * tan_fov
    out = A.Camera.from_buffer_copy(cam)
    for j in range(3):
        out.position[j], out.front[j], out.right[j], out.up[j] = float(position[j]), float(front[j]), float(right[j]), float(up[j])
    return out


def cornell_with_camera(A, api, width, height, camera_of, flags=None):
    """The Cornell box (default: lamp, mirror and glass ball) with the camera camera_of(its own camera) -> A.Camera; the scene's arrays are copies."""
    room = api.cornell_box_scene(A.CB_DEFAULT_SCENE if flags is None else flags, width, height)   # (alive until the copies below are made)
    c = room.c
    copy = lambda T, arr, n: [T.from_buffer_copy(arr[i]) for i in range(n)]
    return CustomScene(A, camera_of(c.camera), copy(A.Shape, c.shapes, c.shape_count), copy(A.Material, c.materials, c.material_count),
                       copy(A.Light, c.lights, c.light_count), copy(A.Surface, c.surfaces, c.surface_count), environment_light=c.environment_light)


def moved_cameras(A, api, width, height):
    """name -> scene: five cameras moved and turned by numbers drawn from SEED.  `back`: the whole box in the middle of the frame; `right` and `up`: turned so
    that the box's bound leaves the frame on one side; `roll`: moved back and rolled about the viewing direction; `away`: turned round, the box behind it."""
    rng = np.random.default_rng(SEED)
    out = {}

    def add(name, back, yaw, pitch, roll, flip=False):
        def camera_of(cam):
            p, f, r, u = (np.array([v[0], v[1], v[2]], np.float64) for v in (cam.position, cam.front, cam.right, cam.up))
            f, r, u = _unit(f), _unit(r), _unit(u)
            front = _unit(f + yaw * r + pitch * u) * (-1.0 if flip else 1.0)
            hint = np.cos(roll) * u + np.sin(roll) * r
            return camera_like(A, cam, p - back * f, front, hint)
        out[name] = cornell_with_camera(A, api, width, height, camera_of)

    add("back", rng.uniform(2.0, 3.0), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.0)
    add("right", rng.uniform(0.0, 0.5), rng.uniform(0.45, 0.6), rng.uniform(-0.05, 0.05), 0.0)
    add("up", rng.uniform(1.0, 2.0), rng.uniform(-0.05, 0.05), rng.uniform(0.45, 0.6), 0.0)
    add("roll", rng.uniform(1.5, 2.5), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 0.7))
    add("away", rng.uniform(0.0, 0.5), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), 0.0, flip=True)
    return out


def inside_camera(A, api, width, height):
    """the Cornell box seen from its own middle (the centre of its surfaces' bound)"""
    def camera_of(cam):
        room = api.cornell_box_scene(A.CB_DEFAULT_SCENE, width, height).c
        pts = np.array([[room.shapes[i].p[q][j] for j in range(3)] for i in range(room.shape_count) if room.shapes[i].kind == A.SHAPE_RECTANGLE for q in range(4)])
        centre = 0.5 * (pts.min(0) + pts.max(0))
        return camera_like(A, cam, centre, [cam.front[0], cam.front[1], cam.front[2]], [cam.up[0], cam.up[1], cam.up[2]])
    return cornell_with_camera(A, api, width, height, camera_of)
