"""GPU (-m gpu): the observation pass (shc_engine_get_observations, shc_fleet_get_observations_device; BatchEngine.observations,
MixedFleet.observations) against its definition: column c of a robot's row is the double the existing getter writes for that robot, leg and
component - unchanged as float64, rounded to nearest even as float32 - and `pad` where the morphology has no such leg or joint.  The pass moves
and casts values, it computes nothing of its own: every comparison is equality of bit patterns (uint64 / uint32 views); a NaN pad is compared
with isnan.  Every engine is driven 30 cycles with non-zero velocity, IMU tilt, tip forces and joint efforts first."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (BODY_FRAMES_DTYPE, LEG_STATE_MSG_DTYPE, OBS_FIELD_NAMES, SHC_ERR_BUSY, SHC_ERR_INVALID_ARG,
                                                     SHC_ERR_UNSUPPORTED, SHC_OK, BatchEngine, ShcError, device_count, obs_spec, observation_columns)
from syropod_highlevel_controller_amd.fleet import MixedFleet
from syropod_highlevel_controller_amd.params import FEAT_SINGLE_STREAM, FEAT_TIP_FORCE
from test_gpu_checkpoint import with_config3_features
from test_gpu_fleet_device_io import LEGS, DOF, ML, MD, host_set, input_set, morphologies, robot_records, views
from test_gpu_resident import config3_params, force_sample, imu_sample, state_bytes

pytestmark = pytest.mark.gpu

ALL = tuple(OBS_FIELD_NAMES)
MSG_MEMBER = {"joint_effort": "joint_efforts", "walker_tip": "walker_tip_position", "target_tip": "target_tip_position", "poser_tip": "poser_tip_position",
              "model_tip": "model_tip_position", "tip_force": "tip_force", "admittance_delta": "admittance_delta", "virtual_stiffness": "virtual_stiffness",
              "stance_progress": "stance_progress", "swing_progress": "swing_progress", "time_to_swing_end": "time_to_swing_end"}
BODY_MEMBERS = ("desired_velocity", "pose_euler", "odom_to_base_link")


def need_gpu():
    if device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")


def drive(eng, p, seed, cycles=30):
    n, L, D = eng.n, eng.legs, eng.dof
    rng = np.random.default_rng(seed)
    lin, ang = rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.8, 0.8, n)
    lin[::4], ang[::4] = 0.0, 0.0   # every fourth robot stands (walk state STOPPED); the others are still STARTING or MOVING after 30 cycles
    eng.set_velocity(lin, ang)
    if p.imu_posing:
        eng.set_imu(*imu_sample(rng, n))
    eng.set_tip_force(force_sample(rng, n, L))
    eff = rng.normal(0, 0.5, (n, L, D))
    for l in range(L):
        eff[:, l, p.leg_dof[l]:] = 0.0
    eng.set_joint_effort(eff.reshape(n, -1))
    eng.step(cycles)
    eng.synchronize()


def msg_fields(msgs, dof):
    """The leg message members an observation field names, as (n, legs, width) arrays."""
    out = {}
    for name, member in MSG_MEMBER.items():
        a = np.ascontiguousarray(msgs[member])
        out[name] = a[:, :, None] if a.ndim == 2 else a[:, :, :dof] if name == "joint_effort" else a
    return out


def engine_reference(eng):
    """Every field from the getters the header names: per-leg fields (n, legs, width), per-robot fields (n, width), float64."""
    n, L, D = eng.n, eng.legs, eng.dof
    q, qd = eng.joints()
    ref = {"q": q.reshape(n, L, D), "qd": qd.reshape(n, L, D)}
    ref.update(msg_fields(eng.leg_state_msgs(), D))
    ref["step_state"] = (eng.leg_state()["leg_status"] & 3).astype(np.float64)[:, :, None]
    pose, _, ws = eng.body_state()
    ref["body_pose"], ref["walk_state"] = pose, ws.astype(np.float64)[:, None]
    _, bf = eng.frame_transforms(legs=False)
    for name in BODY_MEMBERS:
        ref[name] = np.ascontiguousarray(bf[name])
    return ref


def expected(ref, fields, legs, dof, pad):
    cols, width = observation_columns(fields, legs, dof)
    n = len(ref["body_pose"])
    want = np.full((n, width), pad, dtype=np.float64)
    for name in fields:
        a, sl = ref[name], cols[name]
        if a.ndim == 3:
            block = np.full((n, legs, (sl.stop - sl.start) // legs), pad, dtype=np.float64)
            block[:, :a.shape[1], :a.shape[2]] = a
            a = block.reshape(n, -1)
        want[:, sl] = a
    return want


def assert_bits(got, want64, what):
    """got: float64 or float32 (rows, width); want64: the float64 values.  Equal bit for bit; where want is NaN (a NaN pad), NaN."""
    want = want64.astype(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{what}: a NaN pad column holds a number"
    view = np.uint64 if got.dtype == np.float64 else np.uint32
    bad = (np.ascontiguousarray(got).view(view) != np.ascontiguousarray(want).view(view)) & ~nan
    if bad.any():
        worst = float(np.abs(got[bad].astype(np.float64) - want[bad].astype(np.float64)).max())
        print(f"[observations] {what}: {int(bad.sum())} of {bad.size} elements differ in columns {sorted(set(np.argwhere(bad)[:, 1].tolist()))}, max |d| = {worst:.3e}")
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first at (row, column) {tuple(np.argwhere(bad)[0])}"


def device_rows(eng, fields, dtype, rows, width, extra=0, sentinel=1e30, **kw):
    """observations() into columns [5, 5 + width) of a wider device tensor filled with a sentinel (extra > 0) or into a dense one."""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    big = torch.full((rows, width + extra), sentinel, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    eng.observations(fields, out=big[:, 5:5 + width] if extra else big, **kw)
    eng.synchronize()
    return big.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1. the hexapod, every field
@pytest.fixture(scope="module")
def hexapods():
    need_gpu()
    p = config3_params()
    eng = BatchEngine(p, 23)   # 10 robots per wavefront: the last wavefront is partial
    drive(eng, p, 11)
    ref = engine_reference(eng)
    yield eng, ref
    eng.close()


def test_the_drive_leaves_no_field_trivially_zero(hexapods):
    _, ref = hexapods
    flat = [name for name in ALL if not np.any(ref[name] != 0.0)]
    assert not flat, f"all zero after the drive: {flat}"
    assert len(np.unique(ref["step_state"])) > 1 and (ref["stance_progress"] > 0).any() and (ref["swing_progress"] > 0).any()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("first,count", [(0, 23), (7, 11)])   # the whole batch; a range that starts and ends inside a wavefront
def test_hexapod_every_field(hexapods, dtype, first, count):
    eng, ref = hexapods
    want = expected(ref, ALL, 6, 3, 0.0)[first:first + count]
    assert want.shape[1] == 6 * (3 * 3 + 6 * 3 + 5) + 21
    host = eng.observations(ALL, dtype=dtype, first=first, count=count)
    assert host.dtype == np.dtype(dtype)
    assert_bits(host, want, f"host form {dtype} [{first}, {first + count})")
    dev = device_rows(eng, ALL, dtype, count, want.shape[1], first=first, count=count)
    assert dev.tobytes() == host.tobytes(), "the device form differs from the host form"
    # ... and through a row stride: columns [5, 5 + W) of a wider tensor, the rest untouched
    wide = device_rows(eng, ALL, dtype, count, want.shape[1], extra=11, first=first, count=count)
    assert wide[:, 5:5 + want.shape[1]].tobytes() == host.tobytes()
    rest = np.concatenate([wide[:, :5], wide[:, 5 + want.shape[1]:]], axis=1)
    assert (rest == np.array(1e30, dtype=rest.dtype)).all(), "columns outside [0, width) of a row were written"


def test_hexapod_host_form_with_a_row_stride_is_the_library_call(hexapods):
    """The C entry point with on_device = 0 and a row stride: columns [width, row_stride) of the host array keep what they held."""
    eng, ref = hexapods
    fields = ("model_tip", "walk_state", "qd")
    want = expected(ref, fields, 6, 3, 0.0)
    W = want.shape[1]
    out = np.full((23, W + 3), -5.0)
    spec = obs_spec(fields, 6, 3, "float64", W + 3)
    assert eng.L.shc_engine_get_observations(eng.h, 0, 23, C.byref(spec), out.ctypes.data_as(C.c_void_p), 0) == SHC_OK
    assert_bits(out[:, :W], want, "host form with a row stride")
    assert (out[:, W:] == -5.0).all()


# ---------------------------------------------------------------------------------------------------------------- 2. further morphologies
MORPHS = {"8x5": lambda: with_config3_features(synthetic_octopod_params("ripple", 5, 8)),            # 8 robots per wavefront
          "4x4": lambda: synthetic_octopod_params("amble", 4, 4),                                    # 16 per wavefront; no admittance control
          "mixed": lambda: with_config3_features(synthetic_mixed_dof_params("ripple", (3, 5, 4, 3, 5, 4)))}


@pytest.mark.parametrize("morph", list(MORPHS))
def test_further_morphologies_and_padding(morph):
    need_gpu()
    p = MORPHS[morph]()
    eng = BatchEngine(p, 9)    # more than one wavefront of octopods, a partly filled one everywhere
    drive(eng, p, 12)
    ref = engine_reference(eng)
    L, D = eng.legs, eng.dof
    legs, dof = 8, 6           # the row geometry is larger than the robot's (the octopod's legs: equal - 8 is the bound)
    fields = ALL if p.admittance_control else tuple(f for f in ALL if f != "virtual_stiffness")
    if not p.admittance_control:
        assert not ref["admittance_delta"].any()   # zero with admittance control off, as the record
    cols, width = observation_columns(fields, legs, dof)
    got = eng.observations(fields, dtype="float64", legs=legs, dof=dof, pad=0.0)
    assert_bits(got, expected(ref, fields, legs, dof, 0.0), f"{morph} float64, pad 0.0")
    qcols = got[:, cols["q"]].reshape(9, legs, dof)
    assert not qcols[:, L:].view(np.uint64).any() and not qcols[:, :, D:].view(np.uint64).any()   # +0.0 by bits
    got = eng.observations(fields, dtype="float32", legs=legs, dof=dof, pad=float("nan"))
    assert_bits(got, expected(ref, fields, legs, dof, np.nan), f"{morph} float32, pad NaN")
    qcols = got[:, cols["q"]].reshape(9, legs, dof)
    assert np.isnan(qcols[:, :, D:]).all() and np.isnan(qcols[:, L:]).all() and np.isfinite(qcols[:, :L, :D]).all()
    tips = got[:, cols["model_tip"]].reshape(9, legs, 3)
    assert np.isnan(tips[:, L:]).all() and np.isfinite(tips[:, :L]).all()
    # a sub-selection of three fields in shuffled order, on the device, through a row stride
    sub = ("pose_euler", "swing_progress", "qd")
    want = expected(ref, sub, legs, dof, -2.5)
    wide = device_rows(eng, sub, "float32", 9, want.shape[1], extra=11, legs=legs, dof=dof, pad=-2.5)
    assert_bits(wide[:, 5:5 + want.shape[1]], want, f"{morph} sub-selection")
    assert (np.delete(wide, np.s_[5:5 + want.shape[1]], axis=1) == np.float32(1e30)).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the fleet
N = 37
MORPH = (np.arange(N) % 3).astype(np.int32)   # hexapod, octopod, mixed-DOF robot, interleaved


def make_fleets(count):
    need_gpu()
    fleets = [MixedFleet(morphologies(), MORPH) for _ in range(count)]
    assert (fleets[0].max_legs, fleets[0].max_dof) == (ML, MD)
    arrays = input_set(21, N, MORPH)
    for f in fleets:
        host_set(f, arrays)
        f.step(30)
        f.synchronize()
    return fleets


def fleet_reference(fleet):
    """Every field from MixedFleet.outputs() (q, qd, leg messages, body frames, walk state) - body_pose and step_state, which no fleet output
    carries, from the parts' engines - with NaN wherever a robot has no such leg or its morphology no such joint."""
    import torch
    n = fleet.n
    q, qd = (torch.zeros((n, ML, MD), dtype=torch.float64, device="cuda") for _ in range(2))
    ws = torch.zeros(n, dtype=torch.int32, device="cuda")
    msgs = torch.zeros(n * ML * LEG_STATE_MSG_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    body = torch.zeros(n * BODY_FRAMES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fleet.outputs(q=q, qd=qd, walk_state=ws, leg_state_msgs=msgs, body_frames=body)
    fleet.synchronize()
    ref = {"q": q.cpu().numpy(), "qd": qd.cpu().numpy(), "walk_state": ws.cpu().numpy().astype(np.float64)[:, None]}
    assert ref["q"].tobytes() == fleet.joints()[0].tobytes()
    ref.update(msg_fields(msgs.cpu().numpy().view(LEG_STATE_MSG_DTYPE).reshape(n, ML), MD))
    bf = body.cpu().numpy().view(BODY_FRAMES_DTYPE)
    for name in BODY_MEMBERS:
        ref[name] = np.ascontiguousarray(bf[name])
    ref["body_pose"], ref["step_state"] = np.zeros((n, 7)), np.zeros((n, ML, 1))
    for view, ids in views(fleet):
        ref["body_pose"][ids] = view.body_state()[0]
        ref["step_state"][ids, :view.legs, 0] = view.leg_state()["leg_status"] & 3
    for i in range(n):
        L, D = LEGS[int(MORPH[i])], DOF[int(MORPH[i])]
        for name, a in ref.items():
            if a.ndim == 3:
                a[i, L:] = np.nan
                if name in ("q", "qd", "joint_effort"):
                    a[i, :, D:] = np.nan
    return ref


@pytest.fixture(scope="module")
def fleets():
    a, b = make_fleets(2)
    yield a, b
    for f in (a, b):
        f.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fleet_rows_in_the_callers_order(fleets, dtype):
    import torch
    a, _ = fleets
    ref = fleet_reference(a)       # (the fleet's first device I/O call: ids and staging are in place from here on)
    held = a.io_nbytes
    assert held > 0
    want = expected(ref, ALL, ML, MD, np.nan)
    W = want.shape[1]
    tdt = torch.float64 if dtype == "float64" else torch.float32
    big = torch.full((N, W + 11), 1e30, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    a.observations(big[:, 5:5 + W], ALL, pad=float("nan"))
    a.synchronize()
    got = big.cpu().numpy()
    assert_bits(got[:, 5:5 + W], want, f"fleet {dtype}")
    assert (np.delete(got, np.s_[5:5 + W], axis=1) == np.array(1e30, dtype=got.dtype)).all(), "a sentinel column was written"
    assert a.io_nbytes == held, "the observation pass allocated"
    # a learner-sized selection, dense, with a number as pad
    sub = ("q", "qd", "model_tip", "stance_progress", "swing_progress", "body_pose", "desired_velocity")
    dense = torch.full((N, observation_columns(sub, ML, MD)[1]), 1e30, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    a.observations(dense, sub, pad=-2.5)
    a.synchronize()
    want = expected(ref, sub, ML, MD, np.nan)
    want[np.isnan(want)] = -2.5
    assert_bits(dense.cpu().numpy(), want, f"fleet {dtype}, learner-sized selection")
    assert a.io_nbytes == held


def test_fleet_stream_ordering_composes(fleets):
    """Inputs made by torch kernels on a side stream s, order_after(s), set_inputs, step(3), observations, order_before(s), a torch copy on s and
    one s.synchronize() give what the twin gives with a full synchronisation around every call.  (This cannot prove the ordering: a missing
    wait would most likely go unnoticed at this size.  It proves that the calls compose and lose nothing.)"""
    import torch
    a, b = fleets
    fields = ("q", "tip_force", "body_pose", "time_to_swing_end")
    W = observation_columns(fields, ML, MD)[1]
    base = {k: torch.from_numpy(v).cuda() for k, v in input_set(22, N, MORPH).items() if k in ("linear_xy", "angular", "tip_force")}
    big_a, big_b = (torch.full((N, W + 11), 1e30, dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        made = {k: v * 0.5 + 0.125 for k, v in base.items()}
    a.order_after(s)
    a.set_inputs(**made)
    a.step(3)
    a.observations(big_a[:, 5:5 + W], fields, pad=float("nan"))
    a.order_before(s)
    with torch.cuda.stream(s):
        copy = big_a.clone()
    s.synchronize()
    torch.cuda.synchronize()
    b.set_inputs(**made)
    b.synchronize()
    b.step(3)
    b.synchronize()
    b.observations(big_b[:, 5:5 + W], fields, pad=float("nan"))
    b.synchronize()
    assert copy.cpu().numpy().tobytes() == big_b.cpu().numpy().tobytes()
    assert_bits(big_b.cpu().numpy()[:, 5:5 + W], expected(fleet_reference(b), fields, ML, MD, np.nan), "the twin after three more cycles")
    for f in (a, b):
        f.scan_health()        # (the getters store the derived tips, which the auxiliary blobs carry: refreshed on both from the same state)
    assert robot_records(a) == robot_records(b)


# ---------------------------------------------------------------------------------------------------------------- 4. no side effects
def test_an_observation_changes_no_state():
    need_gpu()
    p = config3_params()
    a, b = BatchEngine(p, 23), BatchEngine(p, 23)
    for eng in (a, b):
        drive(eng, p, 13)
    before = state_bytes(a), a.get_aux_state()
    assert before == (state_bytes(b), b.get_aux_state())
    for dtype, kw in (("float64", {}), ("float32", {"first": 7, "count": 11}), ("float32", {"legs": 8, "dof": 6, "pad": float("nan")})):
        assert np.isfinite(a.observations(ALL, dtype=dtype, **kw)[:, :6 * 3]).any()
        assert (state_bytes(a), a.get_aux_state()) == before, "an observation changed a state record or an auxiliary blob"
    for eng in (a, b):
        eng.step(10)
        eng.synchronize()
    assert state_bytes(a) == state_bytes(b) and a.get_aux_state() == b.get_aux_state()
    assert a.joints()[0].tobytes() == b.joints()[0].tobytes()
    for eng in (a, b):
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_engine_refusals_write_nothing(hexapods):
    import torch
    eng, ref = hexapods
    L, n = eng.L, eng.n
    fields = ("q", "body_pose")
    W = 25
    out = torch.full((n, W + 4), 1e30, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr = out.data_ptr()
    call = lambda spec, first=0, count=n, p=ptr, h=eng.h: L.shc_engine_get_observations(h, first, count, None if spec is None else C.byref(spec), p, 1)
    good = lambda **kw: obs_spec(fields, 6, 3, "float64", W + 4, **kw)
    assert call(good(), h=None) == SHC_ERR_INVALID_ARG
    assert call(None) == SHC_ERR_INVALID_ARG
    assert call(good(), p=None) == SHC_ERR_INVALID_ARG
    for bad in (obs_spec((), 6, 3), obs_spec((0, 19), 6, 3), obs_spec(("q", "q"), 6, 3), obs_spec(fields, 6, 3, 2), obs_spec(fields, 5, 3), obs_spec(fields, 6, 2),
                obs_spec(fields, 9, 3), obs_spec(fields, 6, 7), obs_spec(fields, 6, 3, "float64", W - 1)):
        assert call(bad) == SHC_ERR_INVALID_ARG
    s = good()
    s.reserved = 1
    assert call(s) == SHC_ERR_INVALID_ARG
    for first, count in ((-1, 3), (0, n + 1), (n, 1), (5, -1), (n + 1, 0)):
        assert call(good(), first, count) == SHC_ERR_INVALID_ARG, (first, count)
    assert call(good(), p=ptr + 4) == SHC_ERR_INVALID_ARG                                   # float64 needs 8 bytes
    assert call(obs_spec(fields, 6, 3, "float32", 2 * (W + 4)), p=ptr + 2) == SHC_ERR_INVALID_ARG   # float32 needs 4
    assert call(good(), first=n, count=0) == SHC_OK and call(good(), count=0) == SHC_OK     # count = 0: a no-op
    with pytest.raises(ShcError):
        eng.observations(("q", "q"))
    with pytest.raises(ValueError):
        eng.observations(fields, out=out[:5])                                               # rows
    with pytest.raises(ValueError):
        eng.observations(fields, out=out[:, :W - 1])                                        # columns
    with pytest.raises(ValueError):
        eng.observations(fields, out=out.T)                                                 # the elements of a row are not contiguous
    with pytest.raises(ValueError):
        eng.observations(fields, out=np.zeros((n, W)))                                      # a host array
    eng.resident_begin(ring_depth=4, max_cycles=100)
    try:
        assert call(good()) == SHC_ERR_BUSY
    finally:
        eng.resident_end()
    eng.synchronize()
    assert (out.cpu().numpy() == 1e30).all(), "a refused call wrote to the buffer"
    assert call(good()) == SHC_OK                                                           # ... and the handle still works
    eng.synchronize()
    assert_bits(out.cpu().numpy()[:, :W], expected(engine_reference(eng), fields, 6, 3, 0.0), "after the refusals")


def test_unsupported_fields_are_refused():
    import torch
    need_gpu()
    p = default_hexapod_params("tripod")           # no admittance control
    eng = BatchEngine(p, 5)
    eng.step(3)
    out = torch.full((5, 64), 1e30, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    call = lambda fields: eng.L.shc_engine_get_observations(eng.h, 0, 5, C.byref(obs_spec(fields, 6, 3, "float64", 64)), out.data_ptr(), 1)
    assert call(("q", "virtual_stiffness")) == SHC_ERR_UNSUPPORTED       # as shc_engine_get_virtual_stiffness
    with pytest.raises(ShcError):
        eng.virtual_stiffness()
    assert call(("odom_to_base_link",)) == SHC_OK
    eng.set_features(FEAT_TIP_FORCE | FEAT_SINGLE_STREAM)                # odometry off
    eng.synchronize()
    out.fill_(1e30)
    torch.cuda.synchronize()
    assert call(("q", "odom_to_base_link")) == SHC_ERR_UNSUPPORTED
    with pytest.raises(ShcError):
        eng.observations(("odom_to_base_link",))
    eng.synchronize()
    assert (out.cpu().numpy() == 1e30).all()
    assert call(("q", "admittance_delta", "pose_euler")) == SHC_OK       # zeros without admittance control; the Euler angles need no odometry
    eng.synchronize()
    got = out.cpu().numpy()
    assert got[:, :18].tobytes() == eng.joints()[0].tobytes() and not got[:, 18:36].view(np.uint64).any()
    eng.close()


def test_fleet_refusals_write_nothing():
    import torch
    need_gpu()
    a = MixedFleet(morphologies(), MORPH)
    a.step(2)
    a.synchronize()
    L = a.L
    fields = ("qd", "odom_to_base_link")
    W = ML * MD + 7
    out = torch.full((N, W), 1e30, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    call = lambda spec, p=out.data_ptr(), h=a.h: L.shc_fleet_get_observations_device(h, None if spec is None else C.byref(spec), p)
    good = obs_spec(fields, ML, MD, "float32")
    assert call(good, h=None) == SHC_ERR_INVALID_ARG and call(None) == SHC_ERR_INVALID_ARG and call(good, p=None) == SHC_ERR_INVALID_ARG
    assert call(obs_spec(fields, ML - 1, MD, "float32")) == SHC_ERR_INVALID_ARG            # below shc_fleet_shape
    assert call(obs_spec(fields, ML, MD - 1, "float32")) == SHC_ERR_INVALID_ARG
    assert call(obs_spec(fields, ML, MD, "float32", W - 1)) == SHC_ERR_INVALID_ARG
    assert call(obs_spec(("qd", "qd"), ML, MD, "float32")) == SHC_ERR_INVALID_ARG
    assert call(good, p=out.data_ptr() + 2) == SHC_ERR_INVALID_ARG
    assert a.io_nbytes == 0                                                                 # nobody got as far as preparing device I/O
    with pytest.raises(ValueError):
        a.observations(out[:-1], fields)
    with pytest.raises(ValueError):
        a.observations(out.to(torch.float16), fields)
    parts = views(a)
    parts[1][0].set_features(FEAT_TIP_FORCE | FEAT_SINGLE_STREAM)                           # the second part loses its odometry: every part is asked first
    assert call(good) == SHC_ERR_UNSUPPORTED
    a.close()
    a = MixedFleet(morphologies(), MORPH)
    a.step(2)
    a.synchronize()
    hexapods = views(a)[0][0]
    hexapods.resident_begin(ring_depth=4, max_cycles=100)
    try:
        assert L.shc_fleet_get_observations_device(a.h, C.byref(good), out.data_ptr()) == SHC_ERR_BUSY
    finally:
        hexapods.resident_end()
    a.synchronize()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.float32(1e30)).all(), "a refused call wrote to the buffer"
    a.observations(out, fields, pad=float("nan"))                                           # ... and the handle still works
    a.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :ML * MD].reshape(N, ML, MD), a.joints()[1].astype(np.float32), equal_nan=True)
    a.close()
