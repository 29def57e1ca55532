"""GPU (-m gpu): fleet device I/O (shc_fleet_set_inputs_device, shc_fleet_get_outputs_device, the two ordering calls) against its definition,
the host forms: a fleet A is driven through the device forms with torch tensors, a twin B through shc_fleet_set_* / shc_fleet_get_* with host
copies of the same arrays.  Every comparison is byte equality: the feature moves data, it computes nothing.

Fleet: the 23 hexapods (6x3) and 14 octopods (8x5) of tests/test_gpu_fleet_checkpoint.py in its interleaving, with a robot of a third bin (six
legs of 3, 5, 4, 3, 5, 4 joints) behind every fourth of them: 46 robots, every part ends in a partly filled wavefront, the caller's order
differs from every part's, and max_legs x max_dof = 8 x 5 pads two of the three bins in each direction.  Config 3's features are on."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (BODY_FRAMES_DTYPE, HEALTH_NEAR_LIMIT, LEG_FRAMES_DTYPE, LEG_STATE_MSG_DTYPE, ROBOT_HEALTH_DTYPE,
                                                     SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, SHC_ERR_UNSUPPORTED, SHC_OK, BatchEngine, FleetInputs, FleetOutputs,
                                                     ShcError, device_count)
from syropod_highlevel_controller_amd.fleet import MixedFleet
from test_gpu_checkpoint import per_robot, with_config3_features
from test_gpu_fleet_checkpoint import MORPH as MORPH2
from test_gpu_resident import config3_params, state_bytes

pytestmark = pytest.mark.gpu

MORPH = []
for _i, _m in enumerate(MORPH2):
    MORPH.append(int(_m))
    if _i % 4 == 3:
        MORPH.append(2)
MORPH = np.array(MORPH, dtype=np.int32)
N = len(MORPH)
HEX, OCT, MIX = (np.flatnonzero(MORPH == k) for k in range(3))
assert (N, len(HEX), len(OCT), len(MIX)) == (46, 23, 14, 9)
LEGS, DOF = {0: 6, 1: 8, 2: 6}, {0: 3, 1: 5, 2: 5}   # per bin: legs, and the joint slots per leg of the bin's arrays (its longest leg)
ML, MD = 8, 5
SENTINEL = 1e300


def morphologies(rough=False):
    out = [config3_params(), with_config3_features(synthetic_octopod_params("ripple", 5, 8)), with_config3_features(synthetic_mixed_dof_params("ripple"))]
    for p in out:
        p.rough_terrain_mode = 1 if rough else 0
    return out


def make(count=2, rough=False, devices=(0,)):
    if device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    fleets = [MixedFleet(morphologies(rough), MORPH, devices) for _ in range(count)]
    assert (fleets[0].max_legs, fleets[0].max_dof) == (ML, MD)
    return fleets


def views(fleet):
    return [(BatchEngine.view(handle, fleet.params[m], len(ids)), ids) for handle, m, _, ids in fleet.parts()]


def robot_records(fleet):
    """(state record bytes, auxiliary blob bytes) of every robot, read through its part's engine, in the caller's order."""
    out = [None] * fleet.n
    for view, ids in views(fleet):
        s, x = per_robot(state_bytes(view), len(ids)), per_robot(view.get_aux_state(), len(ids))
        for j, i in enumerate(ids):
            out[i] = (s[j], x[j])
    assert all(r is not None for r in out)
    return out


def joint_bytes(fleet):
    q, qd = fleet.joints()
    return q.tobytes() + qd.tobytes()


def input_set(seed, n=N, morph=MORPH):
    """One value of every input for every robot.  The per-leg arrays carry SENTINEL in every entry beyond a robot's bin (legs, dof): it must not
    reach any state.  The joint slots a short leg of the third bin does not have lie inside its bin's (6, 5) and pass through, in both forms."""
    rng = np.random.default_rng(seed)
    d = {"linear_xy": rng.uniform(-0.6, 0.6, (n, 2)), "angular": rng.uniform(-0.8, 0.8, n),
         "imu_orientation_wxyz": rng.normal(0, 0.05, (n, 4)) + np.array([1.7, 0.0, 0.0, 0.0]),      # not normalised
         "imu_angular_velocity": rng.normal(0, 0.05, (n, 3)),
         "pose_translation_velocity": rng.uniform(-0.3, 0.3, (n, 3)), "pose_rotation_velocity": rng.uniform(-0.3, 0.3, (n, 3))}
    force, effort = np.full((n, ML, 3), SENTINEL), np.full((n, ML, MD), SENTINEL)
    for i in range(n):
        L, D = LEGS[int(morph[i])], DOF[int(morph[i])]
        force[i, :L] = np.stack([rng.normal(0, 1, L), rng.normal(0, 1, L), rng.uniform(0, 15, L)], axis=1)
        effort[i, :L, :D] = rng.normal(0, 2, (L, D))
    d["tip_force"], d["joint_effort"] = force, effort
    return {k: np.ascontiguousarray(v) for k, v in d.items()}


def to_device(arrays):
    import torch
    t = {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}
    torch.cuda.synchronize()   # the parts run on streams of their own: the arrays are complete before the call
    return t


def host_set(fleet, a):
    """The definition: the five host setters with the same arrays; a missing member is held."""
    if "linear_xy" in a or "angular" in a:
        fleet.set_velocity(a.get("linear_xy"), a.get("angular"))
    if "imu_orientation_wxyz" in a or "imu_angular_velocity" in a:
        fleet.set_imu(a.get("imu_orientation_wxyz"), a.get("imu_angular_velocity"))
    if "pose_translation_velocity" in a or "pose_rotation_velocity" in a:
        fleet.set_pose_input(a.get("pose_translation_velocity"), a.get("pose_rotation_velocity"))
    if "tip_force" in a:
        fleet.set_tip_force(a["tip_force"])
    if "joint_effort" in a:
        fleet.set_joint_effort(a["joint_effort"])


def both_set(a, b, arrays):
    t = to_device(arrays)
    a.set_inputs(**t)
    host_set(b, arrays)
    a.synchronize()            # ... and stay untouched until the parts have read them
    return t


def assert_same(a, b, what):
    ra, rb = robot_records(a), robot_records(b)
    for i in range(a.n):
        assert ra[i] == rb[i], f"{what}: robot {i} (bin {MORPH[i]}) holds other records after the device form than after the host form"
    sentinel = np.float64(SENTINEL).tobytes()
    assert not any(sentinel in part for rec in ra for part in rec), f"{what}: a padding entry of a per-leg input reached the state"


def inputs_case(rough):
    """A through the device form, B through the host setters, and C - host setters, first set only - to show that the second set is no no-op:
    the velocity, IMU, force and effort inputs are no part of the state record, so they show in the cycles that follow, not right after the set."""
    a, b, c = make(3, rough=rough)
    first = input_set(1)
    both_set(a, b, first)
    host_set(c, first)
    assert_same(a, b, "right after the inputs")
    for f in (a, b, c):
        f.step(40)
    assert_same(a, b, "40 cycles later")
    assert joint_bytes(a) == joint_bytes(b)
    assert joint_bytes(c) == joint_bytes(b)
    second = input_set(2)
    for held in ("linear_xy", "imu_orientation_wxyz", "pose_translation_velocity", "pose_rotation_velocity", "joint_effort"):
        del second[held]
    both_set(a, b, second)
    assert_same(a, b, "after a second set with held members")
    for f in (a, b, c):
        f.step(10)
    assert_same(a, b, "10 cycles after the second set")
    assert joint_bytes(a) == joint_bytes(b)
    assert joint_bytes(c) != joint_bytes(b), "the second input set changed nothing: the comparison above shows nothing"
    for f in (a, b, c):
        f.close()


def test_inputs():
    """Case 1: every input at once, un-normalised quaternions, sentinel padding; then a set with NULL members, whose inputs stay held."""
    inputs_case(rough=False)


def test_inputs_rough_terrain():
    """Case 2: rough_terrain_mode on every bin: the tip forces run touchdown detection, whose step planes are part of the records."""
    inputs_case(rough=True)


def device_buffers(fleet, which=("q", "qd", "walk_state", "leg_state_msgs", "leg_frames", "body_frames", "health")):
    """Buffers for MixedFleet.outputs, every byte 0xAB beforehand."""
    import torch
    n = fleet.n
    size = {"q": n * ML * MD * 8, "qd": n * ML * MD * 8, "walk_state": n * 4, "leg_state_msgs": n * ML * LEG_STATE_MSG_DTYPE.itemsize,
            "leg_frames": n * ML * LEG_FRAMES_DTYPE.itemsize, "body_frames": n * BODY_FRAMES_DTYPE.itemsize, "health": n * ROBOT_HEALTH_DTYPE.itemsize}
    raw = {k: torch.full((size[k],), 0xAB, dtype=torch.uint8, device="cuda") for k in which}
    out = dict(raw)
    for k in ("q", "qd"):
        if k in out:
            out[k] = raw[k].view(torch.float64).view(n, ML, MD)
    if "walk_state" in out:
        out["walk_state"] = raw["walk_state"].view(torch.int32)
    if "leg_frames" in out:
        out["leg_frames"] = raw["leg_frames"].view(torch.float64)   # (record buffers: any element type with the right number of bytes)
    torch.cuda.synchronize()
    return out, raw


def host_outputs(fleet, frame, crit):
    q, qd = fleet.joints()
    lf, bf = fleet.frame_transforms(frame)
    return {"q": q, "qd": qd, "walk_state": fleet.walk_state(), "leg_state_msgs": fleet.leg_state_msgs(), "leg_frames": lf, "body_frames": bf,
            "health": fleet.scan_health(*crit)}


def read_back(fleet, raw):
    fleet.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in raw.items()}


def drive_30(a, b):
    both_set(a, b, input_set(3))
    for f in (a, b):
        f.step(30)


def some_robots_criteria(fleet):
    """NEAR_LIMIT with a threshold between the two middle values of the robots' limit proximities: the lower half of the robots is flagged."""
    prox = np.unique(fleet.scan_health()["min_limit_proximity"])
    assert len(prox) >= 2, "every robot has the same limit proximity: no threshold selects some of them"
    crit = (HEALTH_NEAR_LIMIT, float(0.5 * (prox[len(prox) // 2 - 1] + prox[len(prox) // 2])), 0.0)
    flagged = (fleet.scan_health(*crit)["flags"] & HEALTH_NEAR_LIMIT) != 0
    assert 0 < flagged.sum() < fleet.n
    return crit


def test_outputs():
    """Case 3: every member in one call, into buffers of 0xAB bytes, for both frames and criteria that flag some robots."""
    a, b = make()
    drive_30(a, b)
    crit = some_robots_criteria(b)
    a.scan_health()            # (B's scans refreshed its derived tips: the same on A, for the records compared at the end)
    for frame in ("base_link", "odom_ideal"):
        out, raw = device_buffers(a)
        a.outputs(frame=frame, select=crit[0], near_limit_proximity=crit[1], tip_deviation=crit[2], **out)
        got, want = read_back(a, raw), host_outputs(b, frame, crit)
        for k in want:
            assert got[k] == want[k].tobytes(), f"{k} (frame {frame}) differs from the host getter's array"
        assert np.isnan(want["q"][HEX[0], 6:]).all() and np.isnan(want["q"][HEX[0], :6, 3:]).all() and np.isfinite(want["q"][OCT]).all()
        assert not want["leg_state_msgs"][HEX[0], 6:].tobytes().strip(b"\0")
    assert_same(a, b, "after the getters")
    for f in (a, b):
        f.step(5)
    assert joint_bytes(a) == joint_bytes(b)
    for f in (a, b):
        f.close()


def test_chunking():
    """Case 4: a chunk of five robots walks the 23-robot part in five passes with a tail of three; same bytes, less staging, no later allocation."""
    a, b = make()
    drive_30(a, b)
    crit = some_robots_criteria(b)
    assert a.io_nbytes > 0     # (the inputs were the first device I/O call)
    results, held = [], []
    for chunk in (0, 5):
        a.set_io_chunk(chunk)
        out, raw = device_buffers(a)
        a.outputs(frame="odom_ideal", select=crit[0], near_limit_proximity=crit[1], tip_deviation=crit[2], **out)
        results.append(read_back(a, raw))
        first = a.io_nbytes
        out, raw = device_buffers(a)
        a.outputs(frame="odom_ideal", select=crit[0], near_limit_proximity=crit[1], tip_deviation=crit[2], **out)
        assert read_back(a, raw) == results[-1]
        assert a.io_nbytes == first, "a second call allocated"
        held.append(first)
    assert results[0] == results[1], "the outputs depend on the chunk"
    want = host_outputs(b, "odom_ideal", crit)
    assert all(results[1][k] == want[k].tobytes() for k in want)
    assert 0 < held[1] < held[0]
    for f in (a, b):
        f.close()


def test_ordering_calls():
    """Case 5.  This test CANNOT prove the ordering - a missing wait would most likely go unnoticed at this size; it proves that the calls compose
    and lose nothing: inputs produced by torch kernels on a non-default stream s, order_after(s), set_inputs, step(3), outputs(q), order_before(s),
    a torch copy of q on s, and one s.synchronize() at the end give what the twin on the host route gives."""
    import torch
    a, b = make()
    base = to_device({k: v for k, v in input_set(4).items() if k in ("linear_xy", "angular", "tip_force")})
    s = torch.cuda.Stream()
    out, raw = device_buffers(a, ("q",))
    with torch.cuda.stream(s):
        made = {k: v * 0.5 + 0.125 for k, v in base.items()}
    a.order_after(s)
    a.set_inputs(**made)
    a.step(3)
    a.outputs(q=out["q"])
    a.order_before(s)
    with torch.cuda.stream(s):
        copy = out["q"].clone()
    s.synchronize()
    host_set(b, {k: v.cpu().numpy() for k, v in made.items()})
    b.step(3)
    assert copy.cpu().numpy().tobytes() == b.joints()[0].tobytes()
    a.order_after(None)        # the default stream, as a raw handle too
    a.order_before(0)
    assert_same(a, b, "after the ordered loop")
    for f in (a, b):
        f.close()


def test_split_steps():
    """Case 6: 40 963 hexapods in one part of its own on the device: 4 097 wavefronts, so shc_engine_step splits every step across two internal
    streams.  Device inputs between steps without a synchronise (the second set rides the half streams), then outputs(q, qd)."""
    if device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    import torch
    n = 40963
    morph = np.zeros(n, dtype=np.int32)
    a, b = (MixedFleet([config3_params()], morph) for _ in range(2))
    assert (a.max_legs, a.max_dof) == (6, 3)
    rng = np.random.default_rng(5)
    sets = [{"linear_xy": rng.uniform(-0.6, 0.6, (n, 2)), "angular": rng.uniform(-0.8, 0.8, n),
             "tip_force": np.ascontiguousarray(np.stack([rng.normal(0, 1, (n, 6)), rng.normal(0, 1, (n, 6)), rng.uniform(0, 15, (n, 6))], axis=2)),
             "joint_effort": rng.normal(0, 2, (n, 6, 3))} for _ in range(2)]
    dev = [to_device(x) for x in sets]
    q, qd = (torch.full((n, 6, 3), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    a.step(2)
    a.set_inputs(**dev[0])
    a.step(2)
    a.set_inputs(**dev[1])
    a.step(2)
    a.outputs(q=q, qd=qd)
    a.synchronize()
    b.step(2)
    host_set(b, sets[0])
    b.step(2)
    host_set(b, sets[1])
    b.step(2)
    wq, wqd = b.joints()
    assert q.cpu().numpy().tobytes() == wq.tobytes() and qd.cpu().numpy().tobytes() == wqd.tobytes()
    for f in (a, b):
        f.close()


def test_refusals_change_nothing():
    """Case 7."""
    import torch
    (a,) = make(1)
    L = a.L
    t = to_device(input_set(6))
    a.set_inputs(**t)
    a.step(5)
    a.synchronize()
    out, raw = device_buffers(a)
    ins, outs = FleetInputs(), FleetOutputs()
    ins.angular = t["angular"].data_ptr()
    outs.q = out["q"].data_ptr()
    # a part in resident mode: both directions are busy, and nobody has moved (the records are read once the loop has ended)
    hexapods = views(a)[0][0]
    hexapods.resident_begin(ring_depth=4, max_cycles=100)
    hexapods.resident_end()    # (whatever entering and leaving resident mode itself leaves in the records is in `before`)
    before = robot_records(a)
    hexapods.resident_begin(ring_depth=4, max_cycles=100)
    try:
        assert L.shc_fleet_set_inputs_device(a.h, C.byref(ins)) == SHC_ERR_BUSY
        assert L.shc_fleet_get_outputs_device(a.h, C.byref(outs)) == SHC_ERR_BUSY
        assert L.shc_fleet_order_after_stream(a.h, None) == SHC_ERR_BUSY and L.shc_fleet_order_stream_after(a.h, None) == SHC_ERR_BUSY
        with pytest.raises(ShcError):
            a.set_inputs(angular=t["angular"])
    finally:
        hexapods.resident_end()
    assert robot_records(a) == before
    assert raw["q"].cpu().numpy().tobytes() == b"\xab" * raw["q"].numel()
    # shapes and types
    with pytest.raises(ValueError, match=r"\(46, 8, 3\)"):
        a.set_inputs(tip_force=t["tip_force"][:, :6])
    with pytest.raises(ValueError):
        a.set_inputs(angular=t["angular"].float())
    with pytest.raises(ValueError):
        a.set_inputs(linear_xy=t["linear_xy"].T)
    with pytest.raises(ValueError):
        a.set_inputs(angular=np.zeros(N))                                    # a host array
    with pytest.raises(TypeError):
        a.set_inputs(velocity=t["angular"])
    with pytest.raises(ValueError, match=r"\(46, 8, 5\)"):
        a.outputs(q=torch.zeros(N, 6, 3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        a.outputs(walk_state=torch.zeros(N, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        a.outputs(health=raw["health"][:-32])
    # the struct itself
    get = lambda o: L.shc_fleet_get_outputs_device(a.h, C.byref(o))
    assert get(FleetOutputs()) == SHC_ERR_INVALID_ARG                        # every output NULL
    with pytest.raises(ShcError):
        a.outputs()
    outs = FleetOutputs()
    outs.q, outs.reserved = out["q"].data_ptr(), 1
    assert get(outs) == SHC_ERR_INVALID_ARG
    outs = FleetOutputs()
    outs.leg_frames, outs.frame = raw["leg_frames"].data_ptr(), 7
    assert get(outs) == SHC_ERR_INVALID_ARG
    for member in ("leg_state_msgs", "leg_frames", "body_frames", "health"):
        outs = FleetOutputs()
        setattr(outs, member, raw[member].data_ptr() + 8)                    # records need 16 bytes
        assert get(outs) == SHC_ERR_INVALID_ARG, member
    assert L.shc_fleet_set_io_chunk(a.h, -1) == SHC_ERR_INVALID_ARG
    a.synchronize()
    assert robot_records(a) == before
    assert all(v.cpu().numpy().tobytes() == b"\xab" * v.numel() for v in raw.values()), "a refused call wrote to a buffer"
    # ... and the handle still works
    outs = FleetOutputs()
    outs.q = out["q"].data_ptr()
    assert get(outs) == SHC_OK
    a.synchronize()
    assert out["q"].cpu().numpy().tobytes() == a.joints()[0].tobytes()
    a.close()


def test_no_odometry_passes_through():
    """body_frames or SHC_FRAME_ODOM_IDEAL on a part without SHC_FEAT_ODOMETRY: the part's SHC_ERR_UNSUPPORTED, before anything was written."""
    from syropod_highlevel_controller_amd.params import FEAT_SINGLE_STREAM, FEAT_TIP_FORCE
    (a,) = make(1)
    views(a)[1][0].set_features(FEAT_TIP_FORCE | FEAT_SINGLE_STREAM)
    out, raw = device_buffers(a, ("leg_frames", "body_frames"))
    outs = FleetOutputs()
    outs.body_frames = raw["body_frames"].data_ptr()
    assert a.L.shc_fleet_get_outputs_device(a.h, C.byref(outs)) == SHC_ERR_UNSUPPORTED
    outs = FleetOutputs()
    outs.leg_frames, outs.frame = raw["leg_frames"].data_ptr(), 1
    assert a.L.shc_fleet_get_outputs_device(a.h, C.byref(outs)) == SHC_ERR_UNSUPPORTED
    outs.frame = 0
    assert a.L.shc_fleet_get_outputs_device(a.h, C.byref(outs)) == SHC_OK
    a.synchronize()
    assert raw["body_frames"].cpu().numpy().tobytes() == b"\xab" * raw["body_frames"].numel()
    assert raw["leg_frames"].cpu().numpy().tobytes() == a.frame_transforms("base_link", body=False)[0].tobytes()
    a.close()


def test_a_fleet_over_two_devices_is_refused():
    """Case 7, last item: the four device entry points answer SHC_ERR_UNSUPPORTED; the host forms remain."""
    if device_count() < 2:
        pytest.skip("one device visible: a fleet over two devices cannot be built")
    (a,) = make(1, devices=(0, 1))
    t = to_device(input_set(7))
    out, raw = device_buffers(a, ("q",))
    ins, outs = FleetInputs(), FleetOutputs()
    ins.angular, outs.q = t["angular"].data_ptr(), out["q"].data_ptr()
    assert a.L.shc_fleet_set_inputs_device(a.h, C.byref(ins)) == SHC_ERR_UNSUPPORTED
    assert a.L.shc_fleet_get_outputs_device(a.h, C.byref(outs)) == SHC_ERR_UNSUPPORTED
    assert a.L.shc_fleet_order_after_stream(a.h, None) == SHC_ERR_UNSUPPORTED
    assert a.L.shc_fleet_order_stream_after(a.h, None) == SHC_ERR_UNSUPPORTED
    assert a.io_nbytes == 0
    a.set_velocity(np.zeros((N, 2)), np.zeros(N))
    a.step(1)
    assert np.isfinite(a.joints()[0][OCT]).all()
    a.close()
