"""BASELINE.json configs[2], [3], [4] as the driver-run GPU tests see them (configs[0] and [1]: tests/test_smallpt*.py,
tests/test_parity_gpu.py::test_full_size_properties and bench.py itself).

For every configuration: (a) oracle parity at the configuration's FULL samples per pixel on single tiles of the full-size
frame, selected with tile_first / tile_step -- the oracle honours shards, and one 16 x 16 tile is a second of host time --
with the north star's tolerance RMSE < 1e-3; (b) size-independent properties of a full-size render (finite, clamped,
deterministic, tile renders are cut-outs of the frame, statistics agree with a small render); (c) the multi-device entry of
the C ABI on one GPU.
"""
import os
import subprocess

import numpy as np
import pytest

from helpers import explain_pixel, rmse
from oracle import film_writers as FW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "examples", "bin", "ky_drivers")


def _tile_number(params, tx, ty):
    """Number of the tile at tile column tx, tile row ty (include/kyhip.h: rows rotated by their index)."""
    tiles_x = (params.width + params.tile_w - 1) // params.tile_w
    return ty * tiles_x + (tx - ty) % tiles_x


def _one_tile(A, params, tx, ty):
    p = A.RenderParams.from_buffer_copy(params)
    p.tile_first = _tile_number(params, tx, ty)
    p.tile_step = 1 << 30
    return p


def _tile_parity(A, api, O, scene, params, tiles, tol=1e-3):
    """GPU vs oracle on single tiles of the full-size frame at the frame's full spp.  Returns the RMSE per tile."""
    out = []
    for (tx, ty) in tiles:
        p = _one_tile(A, params, tx, ty)
        g = api.render(scene, p)
        c = O.render(scene, p)
        x0, y0 = tx * params.tile_w, ty * params.tile_h
        gt, ct = g[y0:y0 + params.tile_h, x0:x0 + params.tile_w], c[y0:y0 + params.tile_h, x0:x0 + params.tile_w]
        assert g.sum() == pytest.approx(float(gt.sum())), "pixels outside the selected tile were written"
        fin = np.isfinite(ct).all(axis=2)          # the reference's own NaN samples (DESIGN.md "Non-finite samples")
        assert fin.mean() > 0.99 and np.isfinite(gt).all()
        d = gt[fin].astype(np.float64) - ct[fin]
        rmse = float(np.sqrt(np.mean(d ** 2)))
        # A 16 x 16 tile is a small sample: ONE camera sample that takes another decision than the oracle's (a path through the glass
        # sphere that ends on the light in one arithmetic and next to it in the other: 25 / spp in one pixel) is worth 9e-4 of tile RMSE
        # at 1024 spp, while whole frames sit at 2e-6 ... 2.5e-4.  So the north star's 1e-3 holds for the tile without its (at most two)
        # pixels that are off by more than 5e-3 -- and each pixel exempted that way is examined right here, sample by sample: every
        # differing sample of it must differ first in a discrete decision, or at / after a vertex on a specular or Phong surface
        # (helpers.explain_sample); a pixel that is merely wrong fails.  With those pixels the tile must still meet 2e-3.
        m = np.abs(d).max(axis=1)
        keep = np.ones(d.shape[0], bool)
        ys, xs = np.nonzero(fin)
        for i in np.argsort(m)[-2:]:
            if m[i] > 5e-3:
                keep[i] = False
                kinds = explain_pixel(api, O, scene, params, x0 + int(xs[i]), y0 + int(ys[i]))
                assert sum(kinds.values()) > 0, ("exempted pixel without a differing sample", (tx, ty), int(xs[i]), int(ys[i]))
                print("tile", (tx, ty), "pixel", (x0 + int(xs[i]), y0 + int(ys[i])), "off by %.1e:" % m[i], kinds)
        assert float(np.sqrt(np.mean(d[keep] ** 2))) < tol and rmse < 2 * tol, ((tx, ty), rmse, int((~keep).sum()))
        out.append(rmse)
    return out


def test_c3_veach_full_size(A, api, O):
    """configs[2]: render_mis_scene's scene (ky.cpp:4878-4905), 1280 x 720, 4096 spp, path_tracing_iteration d5 both_mis."""
    W, H, spp = 1280, 720, 4096
    scene = api.mis_scene(W, H)
    params = api.make_params(W, H, spp)
    # tiles on the planks under each light's highlight, on the floor, on the back wall and on a light
    rmse = _tile_parity(A, api, O, scene, params, [(20, 30), (40, 33), (60, 36), (10, 42), (70, 8), (52, 20)])
    print("C3 tile RMSE at 4096 spp:", ["%.2e" % r for r in rmse])
    # the full frame (3.8e9 samples, well under a second of kernel time)
    a = api.render(scene, params)
    assert a.shape == (H, W, 3) and np.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
    # a tile render is a cut-out of the frame, bit for bit (global sample keys, order-independent accumulation)
    t = api.render(scene, _one_tile(A, params, 40, 33))
    assert np.array_equal(t[33 * 16:34 * 16, 40 * 16:41 * 16], a[33 * 16:34 * 16, 40 * 16:41 * 16])
    # statistics: same mean as a quarter-size render of the same scene within Monte-Carlo noise of the small one
    small = api.render(api.mis_scene(W // 4, H // 4), api.make_params(W // 4, H // 4, 256))
    assert abs(float(a.mean()) - float(small.mean())) < 3e-3, (a.mean(), small.mean())
    # all six strategies of the driver at full size, reduced spp: every one finite, and the unbiased ones agree in the mean
    means = {}
    for strat in (A.DIRECT_BSDF, A.DIRECT_LIGHT, A.DIRECT_IDLE, A.DIRECT_BSDF_MIS, A.DIRECT_LIGHT_MIS, A.DIRECT_BOTH_MIS):
        f = api.render(scene, api.make_params(W, H, 64, direct_sample=strat))
        assert np.isfinite(f).all() and f.min() >= 0 and f.max() <= 1
        means[strat] = float(f.mean())
    assert means[A.DIRECT_IDLE] < means[A.DIRECT_BOTH_MIS]
    # (the per-sample identity both_mis = (bsdf_mis + light_mis) / 2 is tests/test_parity_gpu.py::test_mis_strategies_are_linear;
    # film means do not obey it: clamp01 per pixel is not linear)
    assert means[A.DIRECT_IDLE] < min(means[A.DIRECT_BSDF], means[A.DIRECT_LIGHT], means[A.DIRECT_BSDF_MIS], means[A.DIRECT_LIGHT_MIS])


BATCH_LIGHTS = ("CB_LIGHT_POINT", "CB_LIGHT_DIRECTION", "CB_LIGHT_AREA", "CB_LIGHT_ENVIRONMENT")


def test_c4_batch(A, api, O, tmp_path):
    """configs[3]: the render_multiple_scene batch (ky.cpp:4819-4876) at 1024 x 1024, 2048 spp -- four Cornell light
    variants + Veach + a first-hit AOV pass -- through the C++ driver (film_grid_t, integrator->render per cell, BMP out)
    and, frame by frame, against the oracle on single tiles at the full 2048 spp."""
    res, spp = 1024, 2048
    frames = []
    for name in BATCH_LIGHTS:
        frames.append((api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | getattr(A, name), res, res), api.make_params(res, res, spp)))
    veach = api.mis_scene(res, res)
    frames.append((veach, api.make_params(res, res, spp)))
    frames.append((veach, api.make_params(res, res, 1, integrator=A.INTEGRATOR_NORMAL, sampler=A.SAMPLER_DEBUG)))
    # (a) parity at full spp: one tile on the glossy floor near the spheres, one on a wall, for every lit frame
    for i, (scene, params) in enumerate(frames[:5]):
        tiles = [(30, 50), (8, 20)] if i < 4 else [(30, 40), (40, 50)]
        rmse = _tile_parity(A, api, O, scene, params, tiles)
        print("C4 frame %d tile RMSE at 2048 spp:" % i, ["%.2e" % r for r in rmse])
    # (b) the whole batch through the C++ driver; its mosaic must be, byte for byte, the numpy writer's encoding of the grid
    # built through the C ABI from Python (independent writer: oracle/film_writers.py)
    if not os.path.exists(DRIVERS):
        pytest.skip("examples not built")
    out = subprocess.run([DRIVERS, "batch"], cwd=tmp_path, capture_output=True, text=True, check=True).stdout
    assert "Msamples/s" in out
    got = open(tmp_path / "batch.bmp", "rb").read()
    grid = np.zeros((2 * res, 3 * res, 3), np.float32)
    for cell, (scene, params) in enumerate(frames):
        api.render(scene, params, film=grid, origin_px=((cell % 3) * res, (cell // 3) * res))
    assert np.isfinite(grid).all() and grid.min() >= 0 and grid.max() <= 1
    for cell in range(6):
        sub = grid[(cell // 3) * res:(cell // 3 + 1) * res, (cell % 3) * res:(cell % 3 + 1) * res]
        assert sub.mean() > 0.01, cell
    want = FW.bmp_bytes(grid)
    assert len(got) == len(want) == 54 + grid.size
    assert got == want


def test_c5_stress(A, api, O):
    """configs[4]: Cornell 4096 x 4096, 16384 spp, max depth 16.  The whole frame is 2.7e11 samples (tens of seconds on one
    GPU: bench.py --workload stress); here: oracle parity on single tiles at the full 16384 spp, one rank's 1/8 shard of the
    frame at reduced spp with the properties a shard must have, and the frame's statistics against a small render."""
    W = H = 4096
    spp, depth = 16384, 16
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, W, H)
    params = api.make_params(W, H, spp, max_path_depth=depth)
    rmse = _tile_parity(A, api, O, scene, params, [(128, 200), (60, 128), (170, 215)])   # floor, left wall, under the glass sphere
    print("C5 tile RMSE at 16384 spp, depth 16:", ["%.2e" % r for r in rmse])
    # one rank's shard of an 8-GPU run (tiles 3, 11, 19, ...) at 64 spp: 1.3e8 samples
    p64 = api.make_params(W, H, 64, max_path_depth=depth, tile_first=3, tile_step=8)
    a = api.render(scene, p64)
    b = api.render(scene, p64)
    assert np.array_equal(a, b) and np.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
    owned = np.zeros((H // 16, W // 16), bool)
    for t in range(3, (W // 16) * (H // 16), 8):
        row = t // (W // 16)
        owned[row, (t % (W // 16) + row) % (W // 16)] = True
    lit = a.reshape(H // 16, 16, W // 16, 16, 3).sum(axis=(1, 3, 4)) > 0
    assert not (lit & ~owned).any()                  # nothing outside the shard
    assert (lit & owned).sum() > 0.95 * owned.sum()  # (a few tiles of the open front see only the black outside)
    assert abs(owned.sum() - owned.size / 8) <= 1 and owned.any(axis=1).all()   # a comb of diagonals: every tile row is visited
    # statistics of the shard = statistics of the frame = those of a small render (depth 16 too)
    small = api.render(api.cornell_box_scene(A.CB_DEFAULT_SCENE, 256, 256), api.make_params(256, 256, 1024, max_path_depth=depth))
    shard_mean = float(a.reshape(H // 16, 16, W // 16, 16, 3).mean(axis=(1, 3, 4))[owned].mean())
    assert abs(shard_mean - float(small.mean())) < 3e-3, (shard_mean, small.mean())
    # the 32-bit limits of the device code are checked, not overflowed: 4096^2 at 2e6 spp has > 2^32 work items
    lib = A.load_kyhip()
    import ctypes as C
    huge = api.make_params(W, H, 2_000_000, max_path_depth=depth)
    film = np.zeros((8, 8, 3), np.float32)
    assert lib.kyhip_render(0, scene.flat, C.byref(huge), film.ctypes.data_as(C.c_void_p), W) == A.KY_ERR_LIMIT


def test_render_multi_on_one_gpu(A, api):
    """kyhip_render_multi (the multi-GPU render behind the C ABI) with device 0 listed two and three times: shards on the
    device's stream, gather block, ONE de-interleaving add -- bit-identical to the single-device call; and the C++ host
    mirror's integrator_t::set_devices through the same path."""
    for scene, p in ((api.cornell_box_scene(A.CB_DEFAULT_SCENE, 200, 120), api.make_params(200, 120, 24)),
                     (api.mis_scene(97, 61), api.make_params(97, 61, 9, tile_w=8, tile_h=24)),
                     (api.cornell_box_scene(A.CB_DEFAULT_SCENE, 64, 64), api.make_params(64, 64, 5, direct_sample=A.DIRECT_LIGHT, tile_w=32, tile_h=32))):
        single = api.render(scene, p)
        for devices in ([0], [0, 0], [0, 0, 0], [0] * 7):
            multi = api.render_multi(scene, p, devices)
            assert np.array_equal(single, multi), devices
        # additive, and a sub-range of tiles through the multi entry
        twice = api.render_multi(scene, p, [0, 0], film=single.copy())
        assert np.array_equal(twice, single + single)
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 96, 64)
    one = api.render_host_api(scene, 11, 5, 48, A.SAMPLER_RANDOM, 6, 96, 64, device=0)
    three = api.render_host_api(scene, 11, 5, 48, A.SAMPLER_RANDOM, 6, 96, 64, device=-3)   # set_devices({0, 0, 0})
    every = api.render_host_api(scene, 11, 5, 48, A.SAMPLER_RANDOM, 6, 96, 64, device=-1)   # all_devices()
    assert np.array_equal(one, three) and np.array_equal(one, every)
    import ctypes as C
    lib = A.load_kyhip()
    film = np.zeros((64, 96, 3), np.float32)
    p = api.make_params(96, 64, 2)
    assert lib.kyhip_render_multi(None, 1, scene.flat, C.byref(p), film.ctypes.data_as(C.c_void_p), 96) == A.KY_ERR_INVALID_VALUE
    bad = (C.c_int * 2)(0, 99)
    assert lib.kyhip_render_multi(bad, 2, scene.flat, C.byref(p), film.ctypes.data_as(C.c_void_p), 96) == A.KY_ERR_INVALID_VALUE


def test_streams_on_one_device_do_not_race(A, api):
    """Two kyhip_render_tiles_device calls in flight on DIFFERENT streams of one device: the library orders the
    second behind the first on the device, so both images are the ones a lone call produces."""
    import ctypes as C
    import torch
    lib = A.load_kyhip()
    dev = torch.device("cuda", 0)
    scene_a, pa = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 512, 384), api.make_params(512, 384, 48)
    scene_b, pb = api.mis_scene(320, 200), api.make_params(320, 200, 24)
    ref_a, ref_b = api.render(scene_a, pa), api.render(scene_b, pb)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for _ in range(3):
        ta = torch.zeros((lib.kyhip_shard_float_count(C.byref(pa)),), dtype=torch.float32, device=dev)
        tb = torch.zeros((lib.kyhip_shard_float_count(C.byref(pb)),), dtype=torch.float32, device=dev)
        fa = torch.zeros((384, 512, 3), dtype=torch.float32, device=dev)
        fb = torch.zeros((200, 320, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        api._check(lib.kyhip_render_tiles_device(0, scene_a.flat, C.byref(pa), C.c_void_p(ta.data_ptr()), None, 0, C.c_void_p(s1.cuda_stream)))
        api._check(lib.kyhip_render_tiles_device(0, scene_b.flat, C.byref(pb), C.c_void_p(tb.data_ptr()), None, 0, C.c_void_p(s2.cuda_stream)))
        api._check(lib.kyhip_film_add_tiles_device(0, C.byref(pa), C.c_void_p(ta.data_ptr()), C.c_void_p(fa.data_ptr()), 512, C.c_void_p(s1.cuda_stream)))
        api._check(lib.kyhip_film_add_tiles_device(0, C.byref(pb), C.c_void_p(tb.data_ptr()), C.c_void_p(fb.data_ptr()), 320, C.c_void_p(s2.cuda_stream)))
        torch.cuda.synchronize(dev)
        assert np.array_equal(fa.cpu().numpy(), ref_a) and np.array_equal(fb.cpu().numpy(), ref_b)


def test_gpu_film_to_bmp_with_odd_width(A, api, tmp_path):
    """SURVEY 8(f)1 on a GPU film whose width is not a multiple of 4 (the reference's padding quirk): the C++ writer's file
    equals the numpy restatement's bytes; PPM and HDR likewise."""
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 50, 34)
    film = api.render(scene, api.make_params(50, 34, 16))
    for kind, fn in (("bmp", FW.bmp_bytes), ("ppm", FW.ppm_bytes), ("hdr", FW.hdr_bytes)):
        path = str(tmp_path / ("odd." + kind))
        api.store_image(path, film, kind)
        assert open(path, "rb").read() == fn(film), kind
    b = open(tmp_path / "odd.bmp", "rb").read()
    assert len(b) == 54 + 50 * 34 * 3 and int.from_bytes(b[2:6], "little") == 54 + 152 * 34


def _bench_line(cmd, env, cwd):
    import json
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=cwd)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_two_ranks_on_one_gpu(tmp_path):
    """bench.py's N > 1 path end to end (torch.distributed.run, two ranks, shards -> ONE gather -> one add kernel) on a single
    GPU: KY_BENCH_ONE_GPU=1 puts both ranks on cuda:0 and runs the collective over gloo.  The film must be the one a single rank
    renders (the JSON line carries its mean), and the line must keep the contract's fields.  Round 5: the launch mode is the SAME at every N
    (pipelined by default, --no-pipeline for the single-frame rate), both rates are in the line, and so is which device each rank used."""
    import sys
    env = dict(os.environ, KY_BENCH_ONE_GPU="1", MASTER_ADDR="127.0.0.1")
    args = ["--steps", "2", "--warmup", "1", "--workload", "batch", "--spp", "16", "--width", "256", "--no-cpu-baseline", "--full"]
    bench = os.path.join(ROOT, "bench.py")
    torchrun = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(29700 + os.getpid() % 200), bench, "--gpus", "2"]
    j1 = _bench_line([sys.executable, bench] + args, env, tmp_path)
    j2 = _bench_line(torchrun + args, env, tmp_path)
    j3 = _bench_line([sys.executable, bench, "--no-pipeline"] + args, env, tmp_path)
    assert j1["n_gpus"] == 1 and j2["n_gpus"] == 2 and j2["scaling"] == "strong"
    assert j1["film_mean"] == j2["film_mean"] and j1["film_mean"] > 0.01
    # one launch mode for every N: pipelined on two streams unless --no-pipeline; the same film either way
    assert "pipelined" in j2["config"]["parallelism"] and "pipelined" in j1["config"]["parallelism"] and "one stream" in j3["config"]["parallelism"]
    assert j1["launch_mode"].startswith("pipelined") and j2["launch_mode"].startswith("pipelined") and j3["launch_mode"].startswith("single frame")
    assert j3["film_mean"] == j1["film_mean"]
    for j in (j1, j2, j3):   # both rates in every line
        assert j["single_frame"]["value"] > 0 and j["single_frame"]["ms_per_step"] > 0
    assert j3["single_frame"]["value"] == j3["value"]
    for key in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "config", "roofline", "ranks", "communicator"):
        assert key in j2
    assert j2["roofline"]["bound"] == "valu" and j2["roofline"]["contract"]["bound"] == "hbm" and len(j2["config"]["frames"]) == 6
    # who rendered where: one entry per rank, the device each used, what the communicator says about itself
    assert [r["rank"] for r in j2["ranks"]] == [0, 1] and all(r["hip_ordinal"] == 0 and r["name"] for r in j2["ranks"])
    assert j2["communicator"] == {"backend": "gloo", "world": 2} and j1["communicator"]["world"] == 1
    # the roofline that bounds: useful lane-instructions over lane-slots, a fraction by construction
    for j in (j1, j2):
        assert 0 < j["roofline"]["frac"] < 1 and abs(j["roofline"]["frac"] - j["roofline"]["achieved"] / j["roofline"]["peak"]) < 1e-12
        assert len(j["roofline"]["valu_model"]["frames"]) == 6
        assert j["roofline"]["valu_model_exceeds_executed"] in (None, False)


def test_bench_two_ranks_with_masked_devices(tmp_path):
    """The commonest way an 8-GPU launcher starts its ranks: every rank sees ONE device (HIP_VISIBLE_DEVICES), so LOCAL_RANK 1 must not ask for
    cuda:1.  Here both ranks are masked to the box's only GPU and the collective runs over gloo (KY_BENCH_ONE_GPU keeps RCCL, which wants a device
    per rank, out of it; the device pick is the code under test: local_rank % device_count)."""
    import sys
    env = dict(os.environ, KY_BENCH_ONE_GPU="1", MASTER_ADDR="127.0.0.1", HIP_VISIBLE_DEVICES="0")
    args = ["--steps", "1", "--warmup", "1", "--workload", "cornell", "--spp", "16", "--width", "256", "--height", "192", "--no-cpu-baseline"]
    bench = os.path.join(ROOT, "bench.py")
    j1 = _bench_line([sys.executable, bench] + args, env, tmp_path)
    j2 = _bench_line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                      "--master-port", str(29950 + os.getpid() % 40), bench, "--gpus", "2"] + args, env, tmp_path)
    assert j2["n_gpus"] == 2 and j2["film_mean"] == j1["film_mean"] > 0.01
    assert [(r["local_rank"], r["hip_ordinal"], r["visible_devices"], r["mask"]) for r in j2["ranks"]] == [(0, 0, 1, "0"), (1, 0, 1, "0")]


def test_bench_plain_line_and_dumped_film(tmp_path):
    """A plain bench.py run times its K steps and prints the headline, nothing else (the roofline, the single-frame rate and the CPU baseline
    are --full's); --dump-outputs writes the film of the last timed step, the same film on every run with the same arguments."""
    import sys
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--workload", "cornell", "--spp", "16", "--width", "256",
            "--height", "192"]
    j1 = _bench_line(args + ["--dump-outputs", str(tmp_path / "a")], dict(os.environ), tmp_path)
    j2 = _bench_line(args + ["--dump-outputs", str(tmp_path / "b")], dict(os.environ), tmp_path)
    for j in (j1, j2):
        assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0 and j["higher_is_better"] is True and j["dtype"] == "f32"
        assert not ({"roofline", "cpu_baseline", "extra_workloads", "parity_gate"} & set(j))
    a, b = np.load(tmp_path / "a" / "film.npy"), np.load(tmp_path / "b" / "film.npy")
    assert a.shape == (192, 256, 3) and a.dtype == np.float32 and np.array_equal(a, b)
    assert abs(float(a.mean()) - j1["film_mean"]) < 1e-6 and j1["film_mean"] > 0.01


def test_c2_headline_frame_through_the_cpp_driver(A, api, O, tmp_path):
    """configs[1] through the C++ host mirror (`ky_drivers lighting_enum`: film_t, create_integrator(...)->render(), store_image): the
    BMP must be the numpy writer's encoding of the film the C ABI renders from Python, and tiles of the frame at its full 1024 spp
    must match the oracle (the whole frame is bench.py's workload and test_parity_gpu.py::test_full_size_properties's)."""
    scene = api.cornell_box_scene(A.CB_DEFAULT_SCENE, 1024, 768)
    params = api.make_params(1024, 768, 1024)
    rmse = _tile_parity(A, api, O, scene, params, [(32, 24), (20, 40), (45, 38), (5, 5)])   # centre wall, mirror ball, glass ball, a corner
    print("C2 tile RMSE at 1024 spp:", ["%.2e" % r for r in rmse])
    if not os.path.exists(DRIVERS):
        pytest.skip("examples not built")
    out = subprocess.run([DRIVERS, "lighting_enum"], cwd=tmp_path, capture_output=True, text=True, check=True).stdout
    assert "Msamples/s" in out
    got = open(tmp_path / "lighting_enum.bmp", "rb").read()
    assert got == FW.bmp_bytes(api.render(scene, params))


def test_specialised_instantiations_change_nothing(A, api, O, table_kernels, no_boxes):
    """A scene lit by one rectangle area light runs a both_mis kernel compiled without the other light kinds, the environment term, the
    lights loop and the other light shapes (SceneRef::feat); the other five strategies of the iterative integrator have kernels of their
    own instead of the run-time-dispatched one.  Same arithmetic, same random streams: the image must be the same either way
    (kyhip_set_specialisation switches) -- the same bits for the strategy kernels, to the last bit of a pixel for the Cornell-lamp one --
    here on the two Cornell geometries and a room with two lights, for all six strategies."""
    lib = A.load_kyhip()
    from test_random_scenes_gpu import random_room
    scenes = [(api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | A.CB_LIGHT_AREA, 96, 72), 96, 72),
              (api.cornell_box_scene(A.CB_DEFAULT_SCENE, 64, 64), 64, 64)]
    room, kinds = random_room(A, api, O, 4242 + 8, False, 48, 40)       # room 8: a rectangle light and a point light -> not specialised, still equal
    scenes.append((room, 48, 40))
    prev = lib.kyhip_set_specialisation(1)
    try:
        for scene, w, h in scenes:
            for depth, strategy in ((5, A.DIRECT_BOTH_MIS), (16, A.DIRECT_BOTH_MIS), (5, A.DIRECT_LIGHT_MIS), (5, A.DIRECT_BSDF_MIS), (5, A.DIRECT_LIGHT),
                                    (5, A.DIRECT_BSDF), (5, A.DIRECT_IDLE)):
                p = api.make_params(w, h, 96, max_path_depth=depth, direct_sample=strategy, tile_w=16, tile_h=8)
                lib.kyhip_set_specialisation(1)
                on = api.render(scene, p)
                kernel_on = lib.kyhip_last_kernel(0).decode()
                lib.kyhip_set_specialisation(0)
                off = api.render(scene, p)
                kernel_off = lib.kyhip_last_kernel(0).decode()
                assert on.mean() > 0.01 or strategy == A.DIRECT_IDLE
                assert "feat 0" in kernel_off and ("strategy -1" in kernel_off or "strategy 48" in kernel_off), kernel_off
                if not table_kernels:   # KYHIP_JIT=1: every launch on a kernel compiled with all of its scene's facts -- tests/test_jit.py's bound
                    assert np.abs(on - off).max() <= 2e-5, (kernel_on, depth, np.abs(on - off).max())
                elif "feat 0" not in kernel_on:
                    # an instantiation by scene facts (the Cornell lamp): the same expressions, but with code removed around them the
                    # compiler contracts a few multiply-adds differently -- the last bit of some pixels (measured: 6e-8 on 10 % of them)
                    assert scene is not room and np.abs(on - off).max() <= 1.2e-7, (kernel_on, depth, np.abs(on - off).max())
                elif "deferred" in kernel_on and "deferred" not in kernel_off:
                    # light / light_mis on the two-light room: the strategy's kernel defers its shadow rays, the run-time-dispatched one does
                    # not -- the same terms, added to a pixel in fixed point as they resolve instead of in float per vertex
                    assert np.abs(on - off).max() <= 2e-6, (kernel_on, depth, np.abs(on - off).max())
                else:
                    assert np.array_equal(on, off), (strategy, depth)
        # round 3: the other single-light facts and the other integrators' own kernels -- which instantiation runs, and that it changes nothing
        W, H = 64, 48
        for flag, fact in ((A.CB_LIGHT_AREA, "feat 263"), (A.CB_LIGHT_POINT, "feat 8"), (A.CB_LIGHT_DIRECTION, "feat 8"), (A.CB_LIGHT_ENVIRONMENT, "feat 16")):
            scene = api.cornell_box_scene(A.CB_BOTH_SMALL_SPHERES | flag, W, H)
            for integrator in (A.INTEGRATOR_PATH_TRACING_ITERATION, A.INTEGRATOR_DIRECT_LIGHTING, A.INTEGRATOR_SIMPLE_PATH_TRACING_RECURSION,
                               A.INTEGRATOR_PATH_TRACING_RECURSION, A.INTEGRATOR_PATH_TRACING_RECURSION_DEFERED):
                p = api.make_params(W, H, 64, integrator=integrator)
                lib.kyhip_set_specialisation(1)
                on = api.render(scene, p)
                kernel_on = lib.kyhip_last_kernel(0).decode()
                lib.kyhip_set_specialisation(0)
                off = api.render(scene, p)
                kernel_off = lib.kyhip_last_kernel(0).decode()
                assert "integrator %d" % integrator in kernel_on and "strategy 48" in kernel_on, kernel_on
                if integrator != A.INTEGRATOR_SIMPLE_PATH_TRACING_RECURSION:    # (it samples no lights: one kernel for every scene)
                    # (the iterative integrator's lamp kernel also knows the scene's tables for small: 7 + 128)
                    # (... and the environment light's -- 16 + 128, axis planes 1024, plastic on rectangles 2048 --, whose both_mis estimate is estimate_env_both)
                    want = fact
                    if integrator == A.INTEGRATOR_PATH_TRACING_ITERATION:
                        want = {A.CB_LIGHT_AREA: "feat 1415", A.CB_LIGHT_ENVIRONMENT: "feat 3216"}.get(flag, fact)
                    assert not table_kernels or want in kernel_on, (kernel_on, want)
                if integrator != A.INTEGRATOR_PATH_TRACING_ITERATION:
                    assert "strategy -1" in kernel_off, kernel_off
                fin = np.isfinite(on) & np.isfinite(off)
                assert fin.mean() > 0.999 and np.abs(on[fin] - off[fin]).max() <= (2.4e-7 if table_kernels else 2e-5), (kernel_on, kernel_off, np.abs(on[fin] - off[fin]).max())
        lib.kyhip_set_specialisation(1)
        api.render(api.mis_scene(64, 36), api.make_params(64, 36, 8))
        assert "deferred shadow rays" in lib.kyhip_last_kernel(0).decode()
    finally:
        lib.kyhip_set_specialisation(prev)


@pytest.mark.parametrize("seed, fact", [(16, "feat 16"), (20, "feat 8"), (34, "feat 263"), (42, "feat 8"), (78, None)])
def test_recursion_look_up_rides_along(seed, fact, A, api, O, table_kernels):
    """path_tracing_recursion_t's emitter look-up at specular vertices (ky.cpp:4341-4349) in that integrator's own instantiations: the
    look-up ray is carried by the light loop's first traversal (ky_device.hpp, RideAlong) -- under an environment light by the BSDF-sampling
    estimator's nearest-hit scan, otherwise by the shadow-ray scan -- and a hit on a PLASTIC surface draws its lobe number from the path's
    stream (2663).  Rooms with one light each (environment / point / rectangle / directional / sphere), a plastic floor and a mirror or
    glass sphere: the image must equal the run-time-dispatched kernel's (which traces the look-up on its own, as the KATs do) to the last
    bit of a pixel, and the oracle's film."""
    from test_random_scenes_gpu import random_room
    from test_parity_gpu import film_tolerance
    W, H = 48, 40
    scene, kinds = random_room(A, api, O, 4242 + seed, False, W, H)
    assert len(kinds) == 1
    mats = [scene.surfaces[i].material for i in range(len(scene.surfaces))]
    assert mats[0] == 3 and any(m in (4, 5) for m in mats[5:])        # plastic floor; a mirror or glass sphere
    lib = A.load_kyhip()
    p = api.make_params(W, H, 256, integrator=A.INTEGRATOR_PATH_TRACING_RECURSION, tile_w=16, tile_h=8)
    prev = lib.kyhip_set_specialisation(1)
    try:
        on = api.render(scene, p)
        kernel_on = lib.kyhip_last_kernel(0).decode()
        lib.kyhip_set_specialisation(0)
        off = api.render(scene, p)
        kernel_off = lib.kyhip_last_kernel(0).decode()
    finally:
        lib.kyhip_set_specialisation(prev)
    assert "integrator 9" in kernel_on and "strategy 48" in kernel_on and "strategy -1" in kernel_off, (kernel_on, kernel_off)
    if fact and table_kernels:
        assert fact in kernel_on, kernel_on
    fin = np.isfinite(on) & np.isfinite(off)
    d = np.where(fin, np.abs(on - off), 0).max(axis=2)
    if fact:
        assert fin.mean() > 0.999 and d.max() <= (2.4e-7 if table_kernels else 2e-5), (kernel_on, d.max())
    else:
        # the sphere light (radius 0.1): uniform-cone sampling cancels (ky.cpp:798, 1510-1512), so the sampled point moves by 1e-4 of the radius with
        # the compiler's choice of fused multiply-adds -- which differs between the two instantiations' copies of the estimator -- and a sample
        # that grazes the light's own silhouette (quirk 1) flips: measured 4 pixels of 1920 with ONE sample of 256 each (the same samples flip
        # in the KAT build of the riding estimator against the oracle, with the shared traversal on or off; none with the old estimator)
        assert fin.mean() > 0.999 and (d > 2.4e-7).sum() <= 10 and d.max() < 1.0 / 256 + 1e-6, (kernel_on, (d > 2.4e-7).sum(), d.max())
    c = O.render(scene, p)
    ok = np.isfinite(c).all(axis=2) & np.isfinite(on).all(axis=2)
    assert ok.mean() > 0.995 and c[ok].mean() > 0.01
    assert rmse(on[ok], c[ok]) < film_tolerance(256), rmse(on[ok], c[ok])
