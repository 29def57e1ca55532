"""GPU (-m gpu): the resident tensors (shc_engine_resident_post_actions, shc_engine_resident_get_observations_async; BatchEngine
.resident_post_actions, .resident_observations) against their definitions.  Always twins: engines built from the same parameters and driven
identically; A posts the tensor itself, B makes ordinary device posts of float64 arrays cut from the same columns (.double(): static_cast), with
the same `publish`, and NULL for every group the spec does not name.  The feature converts and moves values around an unchanged loop, which has
tests of its own: every comparison is equality of bytes.  Engines run on a torch stream of the test's (stream=), so that torch work queued there
- the op that writes the tensor right before a call, the fill with 1e30 right behind it - is ordered against the engine's own.

Two refusals of the list are not provoked here: "a cycle already published without inputs" cannot be reached through the API
(shc_engine_resident_publish moves the next unposted cycle along with the doorbell), and SHC_ERR_TIMEOUT is the ordinary post's 5 s
back-pressure, which no test waits for."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (SHC_ERR_INVALID_ARG, SHC_ERR_UNSUPPORTED, SHC_OK, BatchEngine, ShcError, act_spec, action_columns,
                                                     obs_spec, observation_columns)
from test_gpu_actions import SENTINEL, SENTINEL_BYTES, action_values, drive_without_effort, need_gpu
from test_gpu_checkpoint import with_config3_features
from test_gpu_observations import drive
from test_gpu_resident import config3_params, state_bytes
from test_gpu_rollout import CANARY, SHUFFLED, SIX

pytestmark = pytest.mark.gpu

VEL = ("linear_xy", "angular")
POSE = ("pose_translation_velocity", "pose_rotation_velocity")
# the specs of consecutive cycles: groups that are not named are held, and the groups' ring positions drift apart
EFFORT_SPECS = (SIX, VEL, SHUFFLED, ("tip_force",), ("joint_effort", "imu_angular_velocity", "imu_orientation"), VEL + ("joint_effort",))
POSE_SPECS = (POSE + VEL, VEL, ("pose_rotation_velocity", "tip_force", "pose_translation_velocity"), ("tip_force",) + VEL, POSE)


class Engines:
    """`count` engines of the same parameters on one torch stream, each driven by `driver` first (Twins of the rollout tests with a driver)."""

    def __init__(self, p, n, seed, count=2, driver=drive, cycles=30, before=None):
        need_gpu()
        import torch
        self.stream = torch.cuda.Stream()
        self.engines = [BatchEngine(p, n, stream=self.stream.cuda_stream) for _ in range(count)]
        for e in self.engines:
            if before:
                before(e)
            driver(e, p, seed, cycles)
        assert len({state_bytes(e) for e in self.engines}) == 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for e in self.engines:
            e.close()


def pose_live(e):   # (the manual-pose group of the state is live from the first pose input on: the kernels that evaluate it)
    e.set_pose_input(np.zeros((e.n, 3)), np.zeros((e.n, 3)))


# name: (parameters, n, driver, before, the specs of the cycles, row geometry (None: the engine's), the tip-force estimate is live)
CASES = {
    "config3_joint_efforts": (config3_params, 250, drive, None, EFFORT_SPECS, None, True),
    "octopods_8x5_joint_efforts": (lambda: synthetic_octopod_params("ripple", 5, 8), 203, drive, None, EFFORT_SPECS, None, True),
    "generic_4x4": (lambda: synthetic_octopod_params("amble", 4, 4), 130, drive, None, EFFORT_SPECS, None, False),
    "mixed_dof": (lambda: with_config3_features(synthetic_mixed_dof_params("ripple")), 37, drive, None, EFFORT_SPECS, None, False),
    "one_hexapod": (config3_params, 1, drive, None, EFFORT_SPECS, None, False),
    "seven_hexapods_8x6_rows": (config3_params, 7, drive, None, EFFORT_SPECS, (8, 6), False),
    "config2_pose_inputs": (lambda: default_hexapod_params("tripod"), 171, drive_without_effort, pose_live, POSE_SPECS, None, False),
}


def row_tensor(rows, dtype, wide, stream, fill=SENTINEL):
    """(the tensor that owns the memory, the (n, A) view the calls get), made on `stream`: dense, or columns [5, 5 + A) of the first n rows of a
    wider (n + 3, A + 16) tensor full of `fill`"""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    n, width = rows.shape
    with torch.cuda.stream(stream):
        big = torch.full((n + 3, width + 16) if wide else (n, width), fill, dtype=tdt, device="cuda")
        view = big[:n, 5:5 + width] if wide else big
        view.copy_(torch.from_numpy(rows).to(tdt).cuda())
    return big, view


def float64_groups(eng, view, fields, legs, dof, stream):
    """The definition's arrays: per group of `fields` the columns of `view` as a dense float64 device array, cut to the engine's legs and joints."""
    import torch
    cols, _ = action_columns(fields, legs, dof)
    n, L, D = eng.n, eng.legs, eng.dof
    out = {}
    with torch.cuda.stream(stream):
        for name in fields:
            a = view[:, cols[name]].to(torch.float64, copy=True)   # (a copy even of a float64 tensor: the tensor is overwritten behind the call)
            if name == "tip_force":
                a = a.reshape(n, legs, 3)[:, :L]
            elif name == "joint_effort":
                a = a.reshape(n, legs, dof)[:, :L, :D]
            out[name] = a.contiguous()
    return out


def ordinary_post(eng, groups, publish):
    """shc_engine_resident_post with on_device = 1: the reference of the definition"""
    ptr = lambda name: groups[name].data_ptr()
    kw = {}
    if "linear_xy" in groups:
        kw["velocity"] = (ptr("linear_xy"), ptr("angular"))
    if "imu_orientation" in groups:
        kw["imu"] = (ptr("imu_orientation"), ptr("imu_angular_velocity"))
    if "pose_translation_velocity" in groups:
        kw["pose_input"] = (ptr("pose_translation_velocity"), ptr("pose_rotation_velocity"))
    for name in ("tip_force", "joint_effort"):
        if name in groups:
            kw[name] = ptr(name)
    return eng.resident_post(on_device=True, publish=publish, **kw)


def post_both(a, b, stream, rows, fields, legs, dof, dtype, wide, publish, keep):
    """One cycle on both twins: A takes the tensor - made on the engine's stream right before the call, filled with 1e30 right behind it, no
    host wait in between -, B the float64 arrays cut from it (which the input stream of B reads: they are complete first)."""
    import torch
    big, view = row_tensor(rows, dtype, wide, stream)
    groups = float64_groups(b, view, fields, legs, dof, stream)
    with torch.cuda.stream(stream):
        ca = a.resident_post_actions(view, fields, publish=publish, legs=legs, dof=dof)
        big.fill_(SENTINEL)
    stream.synchronize()
    cb = ordinary_post(b, groups, publish)
    keep.append(groups)
    assert ca == cb
    return ca


def ring_bytes(eng, cycle):
    return tuple(x.tobytes() for x in eng.resident_joints(cycle))


def end_and_compare(a, b, cycles, what, estimate_live=False):
    assert a.resident_end() == cycles and b.resident_end() == cycles
    sa = state_bytes(a)
    same = sa == state_bytes(b)
    assert same, f"{what}: the state records differ after resident_end"
    for sentinel in SENTINEL_BYTES:
        assert sentinel not in sa, f"{what}: a surplus column or the fill behind a call reached the state"
    if estimate_live:   # (the estimate is really being evaluated: a dead filter would be byte-identical too)
        assert np.abs(a.leg_state()["tip_force"]).max() > 1e-3
    a.step(25), b.step(25)     # the last posted sets are the held inputs now
    same = state_bytes(a) == state_bytes(b)
    assert same, f"{what}: the state records differ 25 ordinary steps later"


# ------------------------------------------------------------------------------------------------------------ 1. twins, byte for byte
@pytest.mark.parametrize("wide", [False, True], ids=["dense", "columns_of_a_wider_tensor"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", list(CASES))
def test_posts_against_ordinary_posts(case, dtype, wide):
    make_params, n, driver, before, specs, geometry, estimate_live = CASES[case]
    p = make_params()
    cycles, depth = 60, 4
    with Engines(p, n, 21, driver=driver, before=before) as t:
        a, b = t.engines
        legs, dof = geometry or (a.legs, a.dof)
        what = f"{case} {dtype}"
        for e in (a, b):
            e.resident_begin(ring_depth=depth, max_cycles=cycles + 10)
        for g, c0 in enumerate(range(0, cycles, depth - 1)):   # groups of ring_depth - 1 cycles: every ring position is reused many times
            c1, keep = min(cycles, c0 + depth - 1), []
            in_launch = g % 2 == 0      # every cycle of the group released by its own post kernel / the group by resident_publish
            for c in range(c0, c1):
                fields = specs[c % len(specs)]
                rows = action_values(1000 + c, n, fields, legs, dof, a.legs, a.dof)
                assert post_both(a, b, t.stream, rows, fields, legs, dof, dtype, wide, in_launch, keep) == c
            if not in_launch:
                a.resident_publish(c1 - c0), b.resident_publish(c1 - c0)
            a.resident_wait(c1), b.resident_wait(c1)
            for c in range(c0, c1):
                same = ring_bytes(a, c) == ring_bytes(b, c)
                assert same, f"{what}: q / qd of cycle {c} differ"
        end_and_compare(a, b, cycles, what, estimate_live)


# ------------------------------------------------------------------------------------------------------------ 2. the header ring wraps
def test_header_ring_wrap():
    """1 100 cycles through post_actions: cycle c writes header c mod 1 024, behind the back-pressure of the ordinary post."""
    import torch
    cycles, n = 1100, 7
    with Engines(config3_params(), n, 22) as t:
        a, b = t.engines
        rng = np.random.default_rng(5)
        with torch.cuda.stream(t.stream):
            rows = torch.from_numpy(rng.uniform(-0.6, 0.6, (cycles, n, 3)).astype(np.float32)).cuda()
            lin, ang = rows[:, :, :2].double().contiguous(), rows[:, :, 2].double().contiguous()
        t.stream.synchronize()
        for e in (a, b):
            e.resident_begin(ring_depth=8, max_cycles=cycles + 10)
        with torch.cuda.stream(t.stream):
            for c in range(cycles):
                assert a.resident_post_actions(rows[c], VEL, publish=True) == c
        for c in range(cycles):
            assert b.resident_post(velocity=(lin[c].data_ptr(), ang[c].data_ptr()), on_device=True, publish=True) == c
        a.resident_wait(cycles), b.resident_wait(cycles)
        same = ring_bytes(a, cycles - 1) == ring_bytes(b, cycles - 1)
        assert same, "the last cycle's joints differ"
        end_and_compare(a, b, cycles, "header ring wrap")


# ------------------------------------------------------------------------------------------------------------ 3. observations are the ring
def expected_rows(eng, cycle, fields, legs, dof, pad, dtype, tips=None):
    """(n, D) of `dtype`: resident_joints(cycle) cast, `tips` (n, L, 3) for model_tip, in the row geometry (legs, dof) with `pad` elsewhere"""
    cols, width = observation_columns(fields, legs, dof)
    n, L, D = eng.n, eng.legs, eng.dof
    q, qd = eng.resident_joints(cycle)
    want = np.zeros((n, width), dtype=dtype)
    for name, values, k, K in (("q", q, D, dof), ("qd", qd, D, dof), ("model_tip", tips, 3, 3)):
        if name in cols:
            block = np.full((n, legs, K), pad, dtype=np.float64)
            block[:, :L, :k] = values.reshape(n, L, k)
            want[:, cols[name]] = block.reshape(n, -1).astype(dtype)
    return want


def read_rows(eng, stream, cycle, fields, dtype, wide, legs=None, dof=None, pad=0.0):
    """resident_observations into a canary-filled tensor on the engine's stream: (the rows, everything around them is intact)"""
    import torch
    legs, dof = eng.legs if legs is None else legs, eng.dof if dof is None else dof
    n, width = eng.n, observation_columns(fields, legs, dof)[1]
    big, view = row_tensor(np.full((n, width), CANARY), dtype, wide, stream, fill=CANARY)
    with torch.cuda.stream(stream):
        assert eng.resident_observations(cycle, fields, out=view, pad=pad, legs=legs, dof=dof) is None
    stream.synchronize()
    got, whole = view.cpu().numpy(), big.cpu().numpy()
    if wide:
        whole[:n, 5:5 + width] = CANARY
    return got, (not wide) or bool((whole == CANARY).all())


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_observations_are_the_ring(dtype):
    """A in resident mode, B the same cycles as launches (set_actions + step: byte-identical, as the resident tests show) - B holds the joints
    of the last cycle, and its observation pass the tips that belong to them."""
    import torch
    n, cycles, depth = 23, 7, 8
    with Engines(config3_params(), n, 23) as t:
        a, b = t.engines
        a.resident_begin(ring_depth=depth, max_cycles=100)
        for c in range(cycles):
            _, view = row_tensor(action_values(2000 + c, n, SIX, 6, 3, 6, 3), "float32", False, t.stream)
            with torch.cuda.stream(t.stream):
                assert a.resident_post_actions(view, SIX, publish=True) == c
                b.set_actions(view, SIX)
                b.step(1)
        a.resident_wait(cycles), b.synchronize()
        last = cycles - 1
        assert tuple(x.tobytes() for x in b.joints()) == ring_bytes(a, last)
        assert len({ring_bytes(a, c) for c in range(cycles)}) == cycles, "the cycles hold the same joints: the comparisons show nothing"
        tips = b.observations(("model_tip",), dtype="float64").reshape(n, 6, 3)
        np_dtype = np.dtype(dtype)
        for c, fields, wide, geometry, pad in ((last, ("q", "qd", "model_tip"), False, (None, None), 0.0), (last, ("model_tip", "qd", "q"), True, (8, 6), -7.25),
                                              (last, ("model_tip",), True, (None, None), 0.0), (2, ("q", "qd"), True, (8, 6), 3.5), (0, ("qd",), False, (None, None), 0.0),
                                              (4, ("qd", "q"), False, (7, 3), -1.0)):
            got, intact = read_rows(a, t.stream, c, fields, dtype, wide, *geometry, pad=pad)
            want = expected_rows(a, c, fields, geometry[0] or 6, geometry[1] or 3, pad, np_dtype, tips)
            assert got.tobytes() == want.tobytes(), f"cycle {c} {fields} {dtype} wide={wide}"
            assert intact, "a column outside [0, width) or a row outside the n robots was written"
        # a new tensor
        with torch.cuda.stream(t.stream):
            made = a.resident_observations(last, dtype=dtype)
        t.stream.synchronize()
        assert tuple(made.shape) == (n, 36) and made.cpu().numpy().tobytes() == expected_rows(a, last, ("q", "qd"), 6, 3, 0.0, np_dtype).tobytes()
        # a read queued before its cycle is published completes once it is published
        _, view = row_tensor(action_values(2100, n, VEL, 6, 3, 6, 3), "float32", False, t.stream)
        with torch.cuda.stream(t.stream):
            assert a.resident_post_actions(view, VEL) == cycles
            b.set_actions(view, VEL)
            b.step(1)
            pending = a.resident_observations(cycles, ("q", "qd"), dtype=dtype)
        assert a.resident_status()[:2] == (cycles, cycles), "the cycle is not released yet"
        a.resident_publish(1)
        t.stream.synchronize()
        a.resident_wait(cycles + 1)
        assert pending.cpu().numpy().tobytes() == expected_rows(a, cycles, ("q", "qd"), 6, 3, 0.0, np_dtype).tobytes()
        # ... and no read has written into the engine
        assert a.resident_end() == cycles + 1
        b.synchronize()
        same = state_bytes(a) == state_bytes(b)
        assert same, "the reads changed the end state"


# ------------------------------------------------------------------------------------------------------------ 4. stream order, no host sync
def test_closed_loop_without_a_host_sync():
    """20 ticks of post -> read -> next actions from the read, everything on the engine's stream.  A never waits on the host and its action
    tensor is overwritten right behind every call; B synchronises between all steps."""
    import torch
    n, ticks = 250, 20
    fields = VEL + ("joint_effort",)
    with Engines(config3_params(), n, 24) as t:
        a, b = t.engines
        s = t.stream

        def policy(obs, tick):   # (n, 36) float32 -> (n, 21) float32, the same torch ops for both
            q, qd = obs[:, :18], obs[:, 18:]
            return torch.cat([0.4 * torch.sin(3.0 * q[:, :2] + 0.1 * tick), 0.5 * torch.cos(2.0 * q[:, 2:3]), 0.5 * qd + 0.05 * q], dim=1)

        results = []
        for eng, synced in ((a, False), (b, True)):
            eng.resident_begin(ring_depth=4, max_cycles=100)
            with torch.cuda.stream(s):
                obs = torch.zeros((n, 36), dtype=torch.float32, device="cuda")
                for tick in range(ticks):
                    act = policy(obs, tick)            # written by a torch op on the engine's stream immediately before the call
                    assert eng.resident_post_actions(act, fields, publish=True) == tick
                    if synced:
                        s.synchronize(), eng.resident_wait(tick + 1)
                    act.fill_(SENTINEL)               # ... and overwritten immediately after it
                    obs = eng.resident_observations(tick)
                    if synced:
                        s.synchronize()
            s.synchronize()
            results.append(obs.cpu().numpy().tobytes())
            eng.resident_wait(ticks)
            results.append(ring_bytes(eng, ticks - 1))
        same = results[0] == results[2] and results[1] == results[3]
        assert same, "the loop without host synchronisation ended elsewhere"
        end_and_compare(a, b, ticks, "closed loop")


# ------------------------------------------------------------------------------------------------------------ 5. beside a loop that fills the chip
def test_full_chip():
    """19 830 hexapods: 1 983 loop wavefronts + the relay leave one compute unit per XCD.  Every kernel of the two calls must be scheduled
    beside them: a post kernel that is not leaves its cycle unreleased, a read kernel that is not a late read - both bounded on the device."""
    import torch
    n, ticks = 19830, 30
    with Engines(config3_params(), n, 25, cycles=6) as t:
        a, b = t.engines
        s = t.stream
        views = [row_tensor(action_values(3000 + tick, n, SIX, 6, 3, 6, 3), "float32", False, s)[1] for tick in range(ticks)]
        s.synchronize()
        a.resident_begin(ring_depth=4, max_cycles=100)     # (behind the tensors: a loop nobody rings for 5 s stops by itself)
        with torch.cuda.stream(s):
            obs = None
            for tick in range(ticks):
                assert a.resident_post_actions(views[tick], SIX, publish=True) == tick     # (a ShcError - SHC_ERR_TIMEOUT - fails the test)
                obs = a.resident_observations(tick)
        a.resident_wait(ticks, timeout_ms=20000)
        s.synchronize()
        assert a.resident_end() == ticks      # (raises for a late read)
        with torch.cuda.stream(s):            # the launch-mode twin, once the chip is free again
            for tick in range(ticks):
                b.set_actions(views[tick], SIX)
                b.step(1)
        b.synchronize()
        q, qd = b.joints()
        same = obs.cpu().numpy().tobytes() == np.concatenate([q, qd], axis=1).astype(np.float32).tobytes()
        assert same, "the last cycle differs from the launch-mode twin"
        same = state_bytes(a) == state_bytes(b)
        assert same, "the end state differs from the launch-mode twin"


# ------------------------------------------------------------------------------------------------------------ 6. refusals change nothing
def test_refusals_change_nothing():
    import torch
    n, depth, max_cycles = 23, 4, 12
    with Engines(config3_params(), n, 26) as t, Engines(config3_params(), n, 26, count=1, driver=drive_without_effort) as t2:
        a, b = t.engines
        (no_effort,) = t2.engines
        lib, s = a.L, t.stream
        width = action_columns(SIX, 6, 3)[1]
        tens = torch.full((n, width + 4), 0.25, dtype=torch.float32, device="cuda")
        t64 = torch.full((n, width + 4), 0.25, dtype=torch.float64, device="cuda")
        out = torch.full((n, 60), CANARY, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        good = lambda f=SIX, **kw: act_spec(f, 6, 3, "float32", **{"row_stride": width + 4, **kw})
        ogood = lambda f=("q", "qd"), **kw: obs_spec(f, 6, 3, "float32", **{"row_stride": 60, **kw})
        cyc = C.c_int64(-7)

        def act(spec, h=a.h, p=None, publish=1):
            return lib.shc_engine_resident_post_actions(h, None if spec is None else C.byref(spec), C.c_void_p(tens.data_ptr() if p is None else p), publish, C.byref(cyc))

        def obs(spec, cycle=0, h=a.h, p=None):
            return lib.shc_engine_resident_get_observations_async(h, cycle, None if spec is None else C.byref(spec), C.c_void_p(out.data_ptr() if p is None else p), 0)

        # an engine that is not in resident mode
        assert act(good()) == SHC_ERR_INVALID_ARG and obs(ogood()) == SHC_ERR_INVALID_ARG
        for e in (a, b):
            e.resident_begin(ring_depth=depth, max_cycles=max_cycles)
        keep = []
        for c in range(2):
            post_both(a, b, s, action_values(4000 + c, n, SIX, 6, 3, 6, 3), SIX, 6, 3, "float32", False, True, keep)
        a.resident_wait(2), b.resident_wait(2)
        status = a.resident_status()
        invalid = {}
        invalid["a NULL spec"] = lambda: act(None)
        invalid["a NULL array"] = lambda: lib.shc_engine_resident_post_actions(a.h, C.byref(good()), None, 1, C.byref(cyc))
        invalid["a NULL engine"] = lambda: act(good(), h=None)
        s0 = good()
        s0.n_fields = 0
        invalid["no field (row_resolve)"] = lambda: act(s0)
        invalid["a repeated field (row_resolve)"] = lambda: act(act_spec(("tip_force", "angular", "linear_xy", "tip_force"), 6, 3))
        s1 = good()
        s1.reserved = 1
        invalid["reserved != 0 (row_resolve)"] = lambda: act(s1)
        invalid["a row stride below the width (row_resolve)"] = lambda: act(good(row_stride=width - 1))
        invalid["legs below the engine's (actions_check)"] = lambda: act(act_spec(SIX, 5, 3, "float32", 60))
        invalid["dof below the engine's (actions_check)"] = lambda: act(act_spec(SIX, 6, 2, "float32", 60))
        invalid["linear_xy without angular"] = lambda: act(good(("linear_xy", "tip_force")))
        invalid["angular without linear_xy"] = lambda: act(good(("angular",)))
        invalid["the IMU orientation without its angular velocity"] = lambda: act(good(("imu_orientation",)))
        invalid["the IMU angular velocity without its orientation"] = lambda: act(good(("imu_angular_velocity",) + VEL))
        invalid["one pose field without the other"] = lambda: act(good(("pose_rotation_velocity",)))
        invalid["an array not aligned to a float"] = lambda: act(good(), p=tens.data_ptr() + 2)
        invalid["an array not aligned to a double"] = lambda: act(act_spec(SIX, 6, 3, "float64", width + 4), p=t64.data_ptr() + 4)
        invalid["observations: a NULL spec"] = lambda: obs(None)
        invalid["observations: a NULL array"] = lambda: lib.shc_engine_resident_get_observations_async(a.h, 0, C.byref(ogood()), None, 0)
        invalid["observations: a NULL engine"] = lambda: obs(ogood(), h=None)
        invalid["observations: a repeated field"] = lambda: obs(ogood(("q", "q")))
        invalid["observations: legs below the engine's"] = lambda: obs(obs_spec(("q",), 5, 3, "float32", 60))
        invalid["observations: dof below the engine's"] = lambda: obs(obs_spec(("q",), 6, 2, "float32", 60))
        invalid["observations: a misaligned array"] = lambda: obs(ogood(), p=out.data_ptr() + 2)
        invalid["observations: a negative cycle"] = lambda: obs(ogood(), cycle=-1)
        invalid["observations: a cycle past max_cycles"] = lambda: obs(ogood(), cycle=max_cycles)
        unsupported = {"the pose fields on an engine that was given none": lambda: act(good(POSE + VEL)),
                       "observations: a field the ring does not hold": lambda: obs(ogood(("q", "walker_tip"))),
                       "observations: a per-robot field": lambda: obs(ogood(("body_pose",)))}
        for code, calls in ((SHC_ERR_INVALID_ARG, invalid), (SHC_ERR_UNSUPPORTED, unsupported)):
            for what, call in calls.items():
                assert call() == code, what
                assert lib.shc_last_error(), what
                assert a.resident_status() == status, f"{what}: the refusal changed resident_status"
        assert cyc.value == -7, "a refused post wrote the cycle index"
        with pytest.raises(ShcError):
            a.resident_post_actions(tens, ("angular", "angular"))
        with pytest.raises(ValueError):
            a.resident_post_actions(tens[:-1], SIX)                    # a row short
        with pytest.raises(ValueError):
            a.resident_post_actions(tens[:, :width - 1], SIX)          # a column short
        with pytest.raises(ValueError):
            a.resident_observations(0, out=out[:, :35])
        # joint efforts on an engine that was given none before resident_begin
        no_effort.resident_begin(ring_depth=depth, max_cycles=max_cycles)
        status2 = no_effort.resident_status()
        assert act(good(("joint_effort",)), h=no_effort.h) == SHC_ERR_UNSUPPORTED
        assert no_effort.resident_status() == status2 and no_effort.resident_end() == 0
        # the next ordinary post gets the cycle it would have got
        post_both(a, b, s, action_values(4002, n, VEL, 6, 3, 6, 3), VEL, 6, 3, "float32", False, True, keep)
        groups = float64_groups(b, tens[:, :3], VEL, 6, 3, s)
        s.synchronize()
        assert ordinary_post(a, groups, False) == 3 and ordinary_post(b, groups, False) == 3
        # the stream rule: a stream-ordered read of the unpublished cycle 3 parks the engine's stream
        with torch.cuda.stream(s):
            qbuf = torch.zeros((n, 18), dtype=torch.float64, device="cuda")
        s.synchronize()     # (of the stream alone: a synchronise of the device would wait for the loops)
        a.resident_joints_async(3, qbuf.data_ptr())
        status = a.resident_status()
        assert act(good(), publish=1) == SHC_ERR_INVALID_ARG and b"stream-ordered read" in lib.shc_last_error()
        assert a.resident_status() == status
        a.resident_publish(1), b.resident_publish(1)
        assert post_both(a, b, s, action_values(4003, n, SIX, 6, 3, 6, 3), SIX, 6, 3, "float64", True, False, keep) == 4
        a.resident_publish(1), b.resident_publish(1)
        a.resident_wait(5), b.resident_wait(5)
        assert qbuf.cpu().numpy().tobytes() == a.resident_joints(3)[0].tobytes()
        # five cycles published: the slot of cycle 0 has been overwritten by cycle 4
        status = a.resident_status()
        assert obs(ogood(), cycle=0) == SHC_ERR_INVALID_ARG and b"overwritten" in lib.shc_last_error()
        want1 = np.concatenate(a.resident_joints(1), axis=1).astype(np.float32)
        assert obs(ogood(), cycle=1) == SHC_OK
        # up to max_cycles: 5 .. 8 released by their posts, 9 .. 11 posted and not released - and then there is no cycle 12
        for c in range(5, max_cycles):
            assert post_both(a, b, s, action_values(4000 + c, n, VEL, 6, 3, 6, 3), VEL, 6, 3, "float32", False, c < 9, keep) == c
        status = a.resident_status()
        assert status[0] == 9
        assert act(good()) == SHC_ERR_INVALID_ARG and b"max_cycles" in lib.shc_last_error()
        assert a.resident_status() == status
        a.resident_publish(3), b.resident_publish(3)
        a.resident_wait(max_cycles), b.resident_wait(max_cycles)
        s.synchronize()
        got = out.cpu().numpy()
        assert got[:, :36].tobytes() == want1.tobytes() and (got[:, 36:] == CANARY).all()
        end_and_compare(a, b, max_cycles, "refusals")
