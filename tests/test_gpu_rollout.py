"""GPU (-m gpu): the rollout tensors (shc_engine_step_k_actions, shc_engine_get_step_k_observations and their fleet forms; BatchEngine /
MixedFleet.step_k_actions, .step_k_observations) against their definitions, the K-cycle launches with float64 arrays.  Always twins: two engines
built from the same parameters and driven identically; A takes step_k with tensor[..., columns].double().contiguous() per group and NULL for every
group the spec does not name, B step_k_actions with the tensor itself.  The feature converts and moves values and calls shc_engine_step_k, which
has tests of its own: every comparison is equality of bytes.  Engines run on a torch stream of the test's (stream=), so that torch work queued
there - the fill of the tensor with 1e30 right behind a call - is ordered against the engine's own."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, SHC_ERR_UNSUPPORTED, SHC_OK, BatchEngine, ShcError, act_spec,
                                                     action_columns, obs_spec, observation_columns)
from syropod_highlevel_controller_amd.params import PARAM_SWING_HEIGHT
from test_gpu_actions import SENTINEL, SENTINEL_BYTES, action_values, need_gpu
from test_gpu_checkpoint import with_config3_features
from test_gpu_fleet_device_io import HEX, MD, MIX, ML, MORPH, N, OCT, make, robot_records, views
from test_gpu_fleet_step_k import k_rows, warm
from test_gpu_observations import drive
from test_gpu_resident import config3_params, state_bytes

pytestmark = pytest.mark.gpu

SIX = ("linear_xy", "angular", "imu_orientation", "imu_angular_velocity", "tip_force", "joint_effort")
SHUFFLED = ("joint_effort", "imu_orientation", "angular", "tip_force", "imu_angular_velocity", "linear_xy")


def rough_params():
    p = default_hexapod_params("tripod")
    p.rough_terrain_mode, p.step_depth = 1, 0.012
    return p


def auto_posing_params():   # a runtime-flag configuration without a batch kernel: shc_engine_step_k takes its serial form
    p = default_hexapod_params("amble")
    p.auto_posing = 1
    return p


# name: (parameters, n, K, fields)
CASES = {
    "config3_joint_efforts": (config3_params, 23, 5, SIX),                      # 10 robots per wavefront: two full robot groups and a partial one
    "octopods_8x5": (lambda: with_config3_features(synthetic_octopod_params("ripple", 5, 8)), 9, 3, SHUFFLED),
    "rough_terrain": (rough_params, 17, 6, ("tip_force", "linear_xy", "angular")),
    "mixed_dof": (lambda: with_config3_features(synthetic_mixed_dof_params("ripple")), 11, 4, SIX),
    "auto_posing_serial_form": (auto_posing_params, 12, 4, ("linear_xy", "angular", "joint_effort")),
    "one_robot_one_cycle": (config3_params, 1, 1, SHUFFLED),
}


class Twins:
    """`count` engines of the same parameters on one torch stream, driven identically."""

    def __init__(self, p, n, seed, count=2, cycles=30):
        need_gpu()
        import torch
        self.stream = torch.cuda.Stream()
        self.engines = [BatchEngine(p, n, stream=self.stream.cuda_stream) for _ in range(count)]
        for e in self.engines:
            drive(e, p, seed, cycles)
        assert len({state_bytes(e) for e in self.engines}) == 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for e in self.engines:
            e.close()


def rollout_values(seed, K, n, fields, legs, dof, L, D, gaps=False):
    """A float64 (K, n, A) set of rows for `fields` in the row geometry (legs, dof): action_values of the action tests per cycle - quaternions not
    normalised, SENTINEL in every column of a leg >= L or a joint >= D.  gaps: every third cycle's tip forces are zero (forces that come and go)."""
    rows = np.stack([action_values(1000 * seed + k, n, fields, legs, dof, L, D) for k in range(K)])
    if gaps and "tip_force" in fields:
        cols, _ = action_columns(fields, legs, dof)
        block = rows[:, :, cols["tip_force"]].reshape(K, n, legs, 3)
        block[::3, :, :L] = 0.0
        rows[:, :, cols["tip_force"]] = block.reshape(K, n, -1)
    return rows


def rollout_tensor(rows, dtype, wide, stream, fill=SENTINEL):
    """(the tensor that owns the memory, the (K, n, A) view the calls get): dense, or columns [5, 5 + A) of the first n rows of every cycle of a
    wider (K, n + 3, A + 16) tensor full of `fill` - a padded row stride and a padded cycle stride."""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    K, n, width = rows.shape
    with torch.cuda.stream(stream):
        big = torch.full((K, n + 3, width + 16) if wide else (K, n, width), fill, dtype=tdt, device="cuda")
        view = big[:, :n, 5:5 + width] if wide else big
        view.copy_(torch.from_numpy(rows).to(tdt).cuda())
    stream.synchronize()
    return big, view


def float64_groups(eng, view, fields, legs, dof, stream):
    """The definition's arrays: per group of `fields` the columns of `view` as a dense float64 device array, cut to the engine's legs and joints."""
    import torch
    cols, _ = action_columns(fields, legs, dof)
    K, n, L, D = view.shape[0], eng.n, eng.legs, eng.dof
    out = {}
    with torch.cuda.stream(stream):
        for name in fields:
            a = view[..., cols[name]].double()
            if name == "tip_force":
                a = a.reshape(K, n, legs, 3)[:, :, :L]
            elif name == "joint_effort":
                a = a.reshape(K, n, legs, dof)[:, :, :L, :D]
            out[name] = a.contiguous()
    return out


def step_k_by_definition(eng, groups, K):
    ptr = lambda name: groups[name].data_ptr() if name in groups else None
    eng.step_k(K, velocity=(ptr("linear_xy"), ptr("angular")) if "linear_xy" in groups else None,
               imu=(ptr("imu_orientation"), ptr("imu_angular_velocity")) if "imu_orientation" in groups else None,
               tip_force=ptr("tip_force"), joint_effort=ptr("joint_effort"))


def ring_bytes(eng, K):
    return [tuple(x.tobytes() for x in eng.step_k_joints(k)) for k in range(K)]


def joint_bits(eng):
    q, qd = eng.joints()
    return q.tobytes() + qd.tobytes()


def assert_twins(a, b, K, what, cycles=3):
    a.synchronize(), b.synchronize()
    sa = state_bytes(a)
    assert sa == state_bytes(b), f"{what}: the state records differ right after the launch"
    assert bytes(a.get_aux_state()) == bytes(b.get_aux_state()), f"{what}: the auxiliary blobs differ"
    ra, rb = ring_bytes(a, K), ring_bytes(b, K)
    for k in range(K):
        assert ra[k] == rb[k], f"{what}: ring slot {k} differs"
    for sentinel in SENTINEL_BYTES:
        assert sentinel not in sa, f"{what}: a surplus column or the fill behind the call reached the state"
    a.step(cycles), b.step(cycles)      # the last cycle's rows are the held inputs now
    assert joint_bits(a) == joint_bits(b), f"{what}: the joints differ {cycles} cycles later"
    assert state_bytes(a) == state_bytes(b), f"{what}: the state records differ {cycles} cycles later"


def two_calls(t, K, fields, legs, dof, dtype, wides, what, gaps=False, seed=5, c=None):
    """Two launches in a row on both twins, B's with no synchronisation in between and a fill of its tensor with 1e30 queued on the engine's
    stream right behind each call; the first launch's ring is kept through step_k_observations (float64, no host wait)."""
    import torch
    a, b = t.engines[:2]
    n, L, D, s = a.n, a.legs, a.dof, t.stream
    sets = [rollout_tensor(rollout_values(seed + i, K, n, fields, legs, dof, L, D, gaps), dtype, wide, s) for i, wide in enumerate(wides)]
    groups = [float64_groups(a, view, fields, legs, dof, s) for _, view in sets]     # (from the tensors as they are now: before any fill)
    s.synchronize()
    step_k_by_definition(a, groups[0], K)
    ring_a = ring_bytes(a, K)
    step_k_by_definition(a, groups[1], K)
    first_ring = torch.full((K, n, 2 * L * D), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for i, (big, view) in enumerate(sets):
            b.step_k_actions(view, fields, legs, dof)
            big.fill_(SENTINEL)
            if i == 0:
                b.step_k_observations(("q", "qd"), out=first_ring)
    b.synchronize()
    host = first_ring.cpu().numpy()
    for k in range(K):
        assert host[k, :, :L * D].tobytes() + host[k, :, L * D:].tobytes() == ring_a[k][0] + ring_a[k][1], f"{what}: ring slot {k} of the first launch differs"
    assert_twins(a, b, K, what)
    if c is not None:
        c.step(2 * K + 3)
        assert joint_bits(c) != joint_bits(a), "the rows changed nothing: the comparison above shows nothing"
    del groups


# ------------------------------------------------------------------------------------------------------------ 1. actions against the definition
@pytest.mark.parametrize("wide", [False, True], ids=["dense", "columns_of_a_wider_tensor"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", list(CASES))
def test_actions_against_step_k(case, dtype, wide):
    make_params, n, K, fields = CASES[case]
    p = make_params()
    with Twins(p, n, 11, count=3) as t:
        a = t.engines[0]
        two_calls(t, K, fields, a.legs, a.dof, dtype, (wide, wide), f"{case} {dtype}", gaps=case == "rough_terrain", c=t.engines[2])


def test_actions_split_streams():
    """41 000 hexapods = 4 100 wavefronts: the launch goes out as two halves on two streams, which read the staged arrays - the second call joins
    them before it overwrites the staging, and the caller's tensor is free right behind each call all the same.  First call dense, second wide."""
    with Twins(config3_params(), 41000, 12, cycles=4) as t:
        two_calls(t, 3, SIX, 6, 3, "float32", (False, True), "split streams")


# ------------------------------------------------------------------------------------------------------------ 2. a row geometry larger than the robot
def test_actions_through_a_larger_row_geometry():
    """Hexapods through 8 x 6 rows: the columns of legs 6, 7 and of joints 3 .. 5 hold 1e30 and none of it reaches the state."""
    with Twins(config3_params(), 23, 13) as t:
        rows = rollout_values(3, 4, 23, SIX, 8, 6, 6, 3)
        cols, width = action_columns(SIX, 8, 6)
        assert width == 10 + 8 * 3 + 8 * 6 and (rows == SENTINEL).sum() == 4 * 23 * (2 * 3 + 2 * 6 + 6 * 3)
        two_calls(t, 4, SIX, 8, 6, "float32", (True, False), "8 x 6 rows, float32")
        two_calls(t, 4, SHUFFLED, 8, 6, "float64", (False, True), "8 x 6 rows, float64", seed=9)


# ------------------------------------------------------------------------------------------------------------ 3. a pending adjusted parameter
def test_actions_with_a_pending_adjusted_parameter():
    """adjust_parameter(swing_height) waits for its loop: the first of the K = 4 cycles takes row 0 through the serial form, the batch kernel the
    other three - shc_engine_step_k's own path, reached with the staged arrays."""
    with Twins(config3_params(), 23, 14, count=3) as t:
        import torch
        a, b, c = t.engines
        for e in (a, b):
            assert e.adjust_parameter(PARAM_SWING_HEIGHT, 0.03) == 0
        two_calls(t, 4, SIX, 6, 3, "float32", (True, False), "pending swing_height")
        # c: the same rows without the change - it must end elsewhere, otherwise the change was lost on the way
        s = t.stream
        for i, wide in enumerate((True, False)):
            _, view = rollout_tensor(rollout_values(5 + i, 4, 23, SIX, 6, 3, 6, 3), "float32", wide, s)
            with torch.cuda.stream(s):
                c.step_k_actions(view, SIX)
        c.step(3)
        assert joint_bits(c) != joint_bits(b), "the adjusted parameter changed nothing"


# ------------------------------------------------------------------------------------------------------------ 4. observations
CANARY = -12345.5


def expected_observations(eng, fields, legs, dof, pad, first, count, dtype):
    """(count, n, D) of `dtype`: step_k_joints(first + k) cast, in the row geometry (legs, dof) with `pad` where the robot has nothing."""
    cols, width = observation_columns(fields, legs, dof)
    n, L, D = eng.n, eng.legs, eng.dof
    want = np.zeros((count, n, width), dtype=dtype)
    for k in range(count):
        q, qd = eng.step_k_joints(first + k)
        for name, values in (("q", q), ("qd", qd)):
            if name in cols:
                block = np.full((n, legs, dof), pad, dtype=np.float64)
                block[:, :L, :D] = values.reshape(n, L, D)
                want[k, :, cols[name]] = block.reshape(n, -1).astype(dtype)
    return want


def check_observations(eng, stream, K, fields, dtype, wide, first, count, legs=None, dof=None, pad=0.0):
    import torch
    legs, dof = eng.legs if legs is None else legs, eng.dof if dof is None else dof
    n, width = eng.n, observation_columns(fields, legs, dof)[1]
    want = expected_observations(eng, fields, legs, dof, pad, first, count, np.dtype(dtype))
    # two more cycles than asked for, before and behind: their rows must keep the canary
    canary = np.full((count + 2, n, width), CANARY)
    big, view = rollout_tensor(canary, dtype, wide, stream, fill=CANARY)
    before = state_bytes(eng)
    with torch.cuda.stream(stream):
        assert eng.step_k_observations(fields, out=view[1:1 + count], first=first, count=count, pad=pad, legs=legs, dof=dof) is None
    eng.synchronize()
    got, whole = view.cpu().numpy(), big.cpu().numpy()
    assert got[1:1 + count].tobytes() == want.tobytes(), f"{fields} {dtype} wide={wide} cycles [{first}, {first + count})"
    assert (got[0] == CANARY).all() and (got[-1] == CANARY).all(), "a row of another cycle was written"
    if wide:
        whole[:, :n, 5:5 + width] = CANARY
        assert (whole == CANARY).all(), "a column outside [0, width) or a row outside the n of a cycle was written"
    assert state_bytes(eng) == before, "the observation wrote into the engine"
    return want


@pytest.fixture(scope="module")
def rolled():
    """Hexapods after a K = 5 launch through step_k_actions."""
    with Twins(config3_params(), 23, 15, count=1) as t:
        (e,) = t.engines
        _, view = rollout_tensor(rollout_values(4, 5, 23, SIX, 6, 3, 6, 3), "float32", False, t.stream)
        e.step_k_actions(view, SIX)
        e.synchronize()
        yield e, t.stream


@pytest.mark.parametrize("wide", [False, True], ids=["dense", "columns_of_a_wider_tensor"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_observations_are_the_ring(rolled, dtype, wide):
    e, s = rolled
    want = check_observations(e, s, 5, ("q", "qd"), dtype, wide, 0, 5)
    assert len({want[k].tobytes() for k in range(5)}) == 5, "the five cycles hold the same joints: the comparison shows nothing"
    check_observations(e, s, 5, ("qd", "q"), dtype, wide, 1, 3)      # a sub-range, the fields the other way round
    check_observations(e, s, 5, ("qd",), dtype, wide, 4, 1)          # the last cycle, one field
    check_observations(e, s, 5, ("q",), dtype, wide, 2, 2, legs=8, dof=6, pad=-7.25)   # pad in a larger geometry


def test_observations_return_a_new_tensor(rolled):
    e, s = rolled
    want = expected_observations(e, ("q", "qd"), 6, 3, 0.0, 1, 3, np.dtype(np.float32))
    import torch
    with torch.cuda.stream(s):
        got = e.step_k_observations(first=1, count=3)
    e.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 23, 36)
    assert got.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_observations_of_a_mixed_dof_robot(dtype):
    """Legs of 3, 5, 4, 3, 5, 4 joints in 6 x 5 arrays: the joints a shorter leg lacks hold what step_k_joints holds there; through 7 x 6 rows the
    seventh leg and the sixth joint hold pad."""
    p = with_config3_features(synthetic_mixed_dof_params("ripple"))
    with Twins(p, 11, 16, count=1) as t:
        (e,) = t.engines
        _, view = rollout_tensor(rollout_values(6, 4, 11, SIX, 6, 5, 6, 5), dtype, True, t.stream)
        e.step_k_actions(view, SIX)
        e.synchronize()
        check_observations(e, t.stream, 4, ("q", "qd"), dtype, False, 0, 4)
        check_observations(e, t.stream, 4, ("q", "qd"), dtype, True, 1, 2, legs=7, dof=6, pad=3.5)


def test_observations_after_a_plain_step_k_and_the_serial_form():
    """The ring is shc_engine_step_k's, whoever launched it: after step_k with float64 arrays, and after the serial form's K single launches."""
    for make_params, fields in ((config3_params, SIX), (auto_posing_params, ("linear_xy", "angular", "joint_effort"))):
        with Twins(make_params(), 12, 17, count=1) as t:
            (e,) = t.engines
            _, view = rollout_tensor(rollout_values(7, 3, 12, fields, 6, 3, 6, 3), "float64", False, t.stream)
            groups = float64_groups(e, view, fields, 6, 3, t.stream)
            t.stream.synchronize()
            step_k_by_definition(e, groups, 3)
            check_observations(e, t.stream, 3, ("q", "qd"), "float32", True, 0, 3)


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def test_engine_refusals_change_nothing():
    import torch
    with Twins(config3_params(), 23, 18, count=1) as t:
        (eng,) = t.engines
        lib, n, s = eng.L, eng.n, t.stream
        K = 3
        fields = ("linear_xy", "angular", "tip_force", "joint_effort")
        width = action_columns(fields, 6, 3)[1]
        _, view = rollout_tensor(rollout_values(8, K, n, fields, 6, 3, 6, 3), "float32", False, s)
        eng.step_k_actions(view, fields)               # the launch whose ring must stay readable
        eng.synchronize()
        ring = ring_bytes(eng, K)
        tens = torch.full((K, n, width + 4), 0.25, dtype=torch.float32, device="cuda")
        t64 = torch.full((K, n, width + 4), 0.25, dtype=torch.float64, device="cuda")
        out = torch.full((K, n, 40), CANARY, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        before, aux_before = state_bytes(eng), bytes(eng.get_aux_state())
        good = lambda f=fields, **kw: act_spec(f, 6, 3, "float32", **{"row_stride": width + 4, **kw})
        ogood = lambda f=("q", "qd"), **kw: obs_spec(f, 6, 3, "float32", **{"row_stride": 40, **kw})

        def act(spec, K=K, p=None, h=None, cycle_stride=0):
            return lib.shc_engine_step_k_actions(eng.h if h is None else h, K, None if spec is None else C.byref(spec),
                                                 C.c_void_p(tens.data_ptr() if p is None else p), cycle_stride)

        def obs(spec, first=0, count=K, p=None, cycle_stride=0):
            return lib.shc_engine_get_step_k_observations(eng.h, first, count, None if spec is None else C.byref(spec),
                                                          C.c_void_p(out.data_ptr() if p is None else p), cycle_stride)
        invalid = {}
        invalid["a NULL spec"] = lambda: act(None)
        invalid["a NULL array"] = lambda: lib.shc_engine_step_k_actions(eng.h, K, C.byref(good()), None, 0)
        invalid["a NULL engine"] = lambda: lib.shc_engine_step_k_actions(None, K, C.byref(good()), C.c_void_p(tens.data_ptr()), 0)
        s0 = good()
        s0.n_fields = 0
        invalid["no field (row_resolve)"] = lambda: act(s0)
        invalid["a repeated field (row_resolve)"] = lambda: act(act_spec(("tip_force", "angular", "linear_xy", "tip_force"), 6, 3))
        s1 = good()
        s1.reserved = 1
        invalid["reserved != 0 (row_resolve)"] = lambda: act(s1)
        invalid["a row stride below the width (row_resolve)"] = lambda: act(good(row_stride=width - 1))
        invalid["legs below the engine's"] = lambda: act(act_spec(fields, 5, 3, "float32", 60))
        invalid["dof below the engine's"] = lambda: act(act_spec(fields, 6, 2, "float32", 60))
        invalid["an array not aligned to a float"] = lambda: act(good(), p=tens.data_ptr() + 2)
        invalid["an array not aligned to a double"] = lambda: lib.shc_engine_step_k_actions(
            eng.h, K, C.byref(act_spec(fields, 6, 3, "float64", width + 4)), C.c_void_p(t64.data_ptr() + 4), 0)
        invalid["K = 0"] = lambda: act(good(), K=0)
        invalid["K = -1"] = lambda: act(good(), K=-1)
        invalid["K = 4097"] = lambda: act(good(), K=4097)
        invalid["a cycle stride below n x the row stride"] = lambda: act(good(), cycle_stride=n * (width + 4) - 1)
        invalid["linear_xy without angular"] = lambda: act(good(("linear_xy", "tip_force")))
        invalid["angular without linear_xy"] = lambda: act(good(("angular",)))
        invalid["the IMU orientation without its angular velocity"] = lambda: act(good(("imu_orientation",)))
        invalid["the IMU angular velocity without its orientation"] = lambda: act(good(("imu_angular_velocity", "linear_xy", "angular")))
        invalid["observations: a NULL spec"] = lambda: obs(None)
        invalid["observations: a NULL array"] = lambda: lib.shc_engine_get_step_k_observations(eng.h, 0, K, C.byref(ogood()), None, 0)
        invalid["observations: a NULL engine"] = lambda: lib.shc_engine_get_step_k_observations(None, 0, K, C.byref(ogood()), C.c_void_p(out.data_ptr()), 0)
        invalid["observations: a repeated field"] = lambda: obs(ogood(("q", "q")))
        invalid["observations: legs below the engine's"] = lambda: obs(obs_spec(("q",), 5, 3, "float32", 40))
        invalid["observations: dof below the engine's"] = lambda: obs(obs_spec(("q",), 6, 2, "float32", 40))
        invalid["observations: a misaligned array"] = lambda: obs(ogood(), p=out.data_ptr() + 2)
        invalid["observations: a negative first cycle"] = lambda: obs(ogood(), first=-1, count=1)
        invalid["observations: no cycle"] = lambda: obs(ogood(), first=0, count=0)
        invalid["observations: a range past the latest launch"] = lambda: obs(ogood(), first=1, count=K)
        invalid["observations: a cycle stride below n x the row stride"] = lambda: obs(ogood(), cycle_stride=n * 40 - 1)
        for what, call in invalid.items():
            assert call() == SHC_ERR_INVALID_ARG, what
            assert lib.shc_last_error(), what
        unsupported = {"pose_translation_velocity": lambda: act(good(("pose_translation_velocity", "linear_xy", "angular"))),
                       "pose_rotation_velocity": lambda: act(good(("pose_rotation_velocity",))),
                       "observations: a field the ring does not hold": lambda: obs(ogood(("q", "walker_tip"))),
                       "observations: a per-robot field": lambda: obs(ogood(("body_pose",)))}
        for what, call in unsupported.items():
            assert call() == SHC_ERR_UNSUPPORTED, what
        # (K-deep staging of 2 GiB or more needs a large batch: test_staging_bound_of_a_large_batch)
        # what the Python layer refuses itself
        with pytest.raises(TypeError, match="device arrays only"):
            eng.step_k_actions(tens.cpu().numpy(), fields)
        with pytest.raises(TypeError, match="device arrays only"):
            eng.step_k_observations(out=out.cpu().numpy())
        with pytest.raises(ValueError):
            eng.step_k_actions(tens[:, :-1], fields)                   # a row short
        with pytest.raises(ValueError):
            eng.step_k_actions(tens[:, :, :width - 1], fields)         # a column short
        with pytest.raises(ValueError):
            eng.step_k_actions(tens[0], fields)                        # two dimensions
        with pytest.raises(ValueError):
            eng.step_k_actions(tens.transpose(1, 2), fields)
        with pytest.raises(ShcError):
            eng.step_k_actions(tens, ("angular", "angular"))
        eng.synchronize()
        assert state_bytes(eng) == before and bytes(eng.get_aux_state()) == aux_before, "a refused call changed the state"
        assert ring_bytes(eng, K) == ring, "a refused call changed the ring"
        assert (out.cpu().numpy() == CANARY).all(), "a refused observation wrote"
        # resident mode
        eng.resident_begin(ring_depth=4, max_cycles=100)
        eng.resident_end()         # (whatever entering and leaving resident mode itself leaves in the records is in `before`)
        before = state_bytes(eng)
        eng.resident_begin(ring_depth=4, max_cycles=100)
        try:
            assert act(good()) == SHC_ERR_BUSY
            assert obs(ogood()) == SHC_ERR_BUSY
        finally:
            eng.resident_end()
        eng.synchronize()
        assert state_bytes(eng) == before, "a call refused in resident mode changed the state"
        assert ring_bytes(eng, K) == ring, "the previous ring is no longer readable"
        assert act(good()) == SHC_OK and obs(ogood()) == SHC_OK        # ... and the handle still works
        eng.synchronize()


def test_staging_bound_of_a_large_batch():
    """65 536 hexapods x 4 096 cycles: the output ring alone (3 planes x 16 B x 65 536+ slots x 4 096) is far above 2 GiB, and so is the staging of
    the joint efforts (18 doubles a robot and cycle: 38 GB) - refused before anything is allocated or read (the array is one row long)."""
    need_gpu()
    import torch
    eng = BatchEngine(config3_params(), 65536)
    try:
        tens = torch.zeros((1, 65536, 18), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        before = state_bytes(eng)
        spec = act_spec(("joint_effort",), 6, 3, "float32")
        assert eng.L.shc_engine_step_k_actions(eng.h, 4096, C.byref(spec), C.c_void_p(tens.data_ptr()), 0) == SHC_ERR_INVALID_ARG
        assert b"2 GiB" in eng.L.shc_last_error()
        # 100 cycles: the ring (6 554 wavefronts x 64 slots x 48 B x 100 = 2.01e9 B) stays below 2^31, the staging of all six groups
        # (100 x 65 536 x 46 doubles = 2.41e9 B) does not
        wide = act_spec(SIX, 6, 3, "float32")
        assert eng.L.shc_engine_step_k_actions(eng.h, 100, C.byref(wide), C.c_void_p(tens.data_ptr()), 0) == SHC_ERR_INVALID_ARG
        assert b"staging" in eng.L.shc_last_error()
        assert state_bytes(eng) == before
    finally:
        eng.close()


def test_an_engine_still_starting_up_is_refused():
    need_gpu()
    import torch
    eng = BatchEngine(config3_params(), 5)
    try:
        eng.begin_direct_startup()
        tens = torch.zeros((2, 5, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        spec = act_spec(("linear_xy", "angular"), 6, 3, "float32")
        assert eng.L.shc_engine_step_k_actions(eng.h, 2, C.byref(spec), C.c_void_p(tens.data_ptr()), 0) == SHC_ERR_UNSUPPORTED
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ 6. fleet
FLEET_FIELDS = {"linear_xy": "linear_xy", "angular": "angular", "imu_orientation": "imu_orientation_wxyz", "imu_angular_velocity": "imu_angular_velocity",
                "tip_force": "tip_force", "joint_effort": "joint_effort"}


def fleet_rows(seed, K, fields):
    """k_rows of the fleet step_k tests (the K-deep float64 record arrays, padded to 8 x 5) as one (K, N, A) row set, 1e30 in the padded entries."""
    arrays = k_rows(seed, K, tuple(FLEET_FIELDS[f] for f in fields))
    cols, width = action_columns(fields, ML, MD)
    rows = np.zeros((K, N, width))
    for name in fields:
        a = arrays[FLEET_FIELDS[name]].reshape(K, N, -1).copy()
        a[a > 1e200] = SENTINEL
        rows[:, :, cols[name]] = a
    return rows


def fleet_groups(view, fields):
    """The float64 record arrays MixedFleet.step_k takes, cut out of the tensor."""
    cols, _ = action_columns(fields, ML, MD)
    K = view.shape[0]
    shape = {"angular": (K, N), "tip_force": (K, N, ML, 3), "joint_effort": (K, N, ML, MD)}
    return {FLEET_FIELDS[name]: view[..., cols[name]].double().contiguous().reshape(shape.get(name, (K, N, -1))) for name in fields}


def fleet_ring(fleet, K):
    import torch
    q, qd = (torch.zeros((K, N, ML, MD), dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    fleet.step_k_joints(0, K, q=q, qd=qd)
    fleet.synchronize()
    return q.cpu().numpy(), qd.cpu().numpy()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fleet(dtype):
    import torch
    a, b = make(2)
    try:
        for f in (a, b):
            warm(f)
        K = 4
        default = torch.cuda.current_stream()
        held = None
        for round_, (fields, wide) in enumerate(((SIX, True), (SHUFFLED, False), (("tip_force", "linear_xy", "angular"), True))):
            big, view = rollout_tensor(fleet_rows(3 + round_, K, fields), dtype, wide, default)
            groups = fleet_groups(view, fields)
            torch.cuda.synchronize()
            a.step_k(K, **groups)
            b.step_k_actions(view, fields)
            b.order_before(default)
            big.fill_(SENTINEL)            # the parts have read the tensor: it may be overwritten behind order_before
            a.synchronize(), b.synchronize()
            what = f"fleet {dtype}, round {round_}"
            ra, rb = robot_records(a), robot_records(b)
            for i in range(N):
                assert ra[i] == rb[i], f"{what}: robot {i} (bin {MORPH[i]}) holds other records than its twin"
            assert not any(sentinel in part for rec in rb for part in rec for sentinel in SENTINEL_BYTES), f"{what}: a padded column reached the state"
            (qa, qda), (qb, qdb) = fleet_ring(a, K), fleet_ring(b, K)
            assert qa.tobytes() == qb.tobytes() and qda.tobytes() == qdb.tobytes(), f"{what}: the rings differ"
            # observations against step_k_joints: NaN there, pad here
            pad = -3.0
            for first, count, owide in ((0, K, False), (1, 2, True)):
                canary = np.full((count + 2, N, 2 * ML * MD), CANARY)
                obig, oview = rollout_tensor(canary, dtype, owide, default, fill=CANARY)
                b.step_k_observations(("qd", "q"), out=oview[1:1 + count], first=first, pad=pad)
                b.synchronize()
                got = oview.cpu().numpy()
                want = np.concatenate([np.where(np.isnan(x), pad, x)[first:first + count].reshape(count, N, -1) for x in (qdb, qb)], axis=2)
                assert got[1:1 + count].tobytes() == want.astype(got.dtype).tobytes(), f"{what}: observations of cycles [{first}, {first + count})"
                assert (got[0] == CANARY).all() and (got[-1] == CANARY).all()
                if owide:
                    whole = obig.cpu().numpy()
                    whole[:, :N, 5:5 + 2 * ML * MD] = CANARY
                    assert (whole == CANARY).all()
                q0 = got[1, :, ML * MD:].reshape(N, ML, MD)
                assert (q0[HEX[0], 6:] == pad).all() and (q0[HEX[0], :6, 3:] == pad).all() and (q0[MIX[0], 6:] == pad).all() and (q0[OCT] != pad).all()
            rb2 = robot_records(b)
            assert rb2 == rb, "an observation wrote into a part"
            if round_ == 0:
                held = b.io_nbytes         # the first call of this K and these groups (all six) has allocated the staging,
                assert held == a.io_nbytes and held > 0   # and shc_fleet_io_bytes counts it as it counts shc_fleet_step_k's
            else:
                assert b.io_nbytes == held, "a later call with the same K and no more groups allocated"
            a.step(3), b.step(3)
            assert a.joints()[0].tobytes() == b.joints()[0].tobytes()
    finally:
        a.close(), b.close()


def test_fleet_refusals():
    import torch
    (a,) = make(1)
    try:
        warm(a)
        lib, K = a.L, 2
        fields = ("linear_xy", "angular", "tip_force")
        width = action_columns(fields, ML, MD)[1]
        tens = torch.full((K, N, width), 0.25, dtype=torch.float32, device="cuda")
        out = torch.full((K, N, 2 * ML * MD), CANARY, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        before = robot_records(a)
        good, ogood = act_spec(fields, ML, MD, "float32"), obs_spec(("q", "qd"), ML, MD, "float32")
        act = lambda spec, K=K, p=None, cs=0: lib.shc_fleet_step_k_actions_device(a.h, K, C.byref(spec), C.c_void_p(tens.data_ptr() if p is None else p), cs)
        obs = lambda spec, first=0, count=K, cs=0: lib.shc_fleet_get_step_k_observations_device(a.h, first, count, C.byref(spec), C.c_void_p(out.data_ptr()), cs)
        assert obs(ogood) == SHC_ERR_INVALID_ARG                              # no K-cycle launch yet
        assert lib.shc_fleet_step_k_actions_device(a.h, K, None, C.c_void_p(tens.data_ptr()), 0) == SHC_ERR_INVALID_ARG
        assert lib.shc_fleet_step_k_actions_device(a.h, K, C.byref(good), None, 0) == SHC_ERR_INVALID_ARG
        assert act(act_spec(fields, ML - 1, MD, "float32")) == SHC_ERR_INVALID_ARG     # below the fleet's shape
        assert act(act_spec(fields, ML, MD - 1, "float32")) == SHC_ERR_INVALID_ARG
        assert act(good, K=0) == SHC_ERR_INVALID_ARG and act(good, K=4097) == SHC_ERR_INVALID_ARG
        assert act(good, cs=N * width - 1) == SHC_ERR_INVALID_ARG
        assert act(good, p=tens.data_ptr() + 2) == SHC_ERR_INVALID_ARG
        assert act(act_spec(("linear_xy", "tip_force"), ML, MD, "float32")) == SHC_ERR_INVALID_ARG
        assert act(act_spec(("imu_orientation",), ML, MD, "float32")) == SHC_ERR_INVALID_ARG
        assert act(act_spec(("pose_rotation_velocity",), ML, MD, "float32")) == SHC_ERR_UNSUPPORTED
        assert obs(obs_spec(("q", "tip_force"), ML, MD, "float32")) == SHC_ERR_UNSUPPORTED
        with pytest.raises(TypeError, match="device arrays only"):
            a.step_k_actions(tens.cpu().numpy(), fields)
        assert robot_records(a) == before
        hexapods = views(a)[0][0]
        hexapods.resident_begin(ring_depth=4, max_cycles=100)
        hexapods.resident_end()    # (whatever entering and leaving resident mode itself leaves in the records is in `before`)
        before = robot_records(a)
        hexapods.resident_begin(ring_depth=4, max_cycles=100)
        try:
            assert act(good) == SHC_ERR_BUSY and obs(ogood) == SHC_ERR_BUSY
        finally:
            hexapods.resident_end()
        assert robot_records(a) == before, "a call refused for one part changed another"
        assert act(good) == SHC_OK
        assert obs(ogood, first=1, count=2) == SHC_ERR_INVALID_ARG            # a range past the latest launch
        assert obs(ogood, first=0, count=0) == SHC_ERR_INVALID_ARG
        assert obs(ogood, cs=N * 2 * ML * MD - 1) == SHC_ERR_INVALID_ARG
        assert obs(ogood) == SHC_OK
        a.synchronize()
        assert not (out.cpu().numpy() == CANARY).any()
    finally:
        a.close()
