"""GPU (-m gpu): fleet step_k (shc_fleet_step_k, shc_fleet_get_step_k_joints_device) against its definition: a fleet A runs K cycles per launch
from K-deep torch tensors in the caller's order, a twin B runs `for k: set inputs (row k); step(1); read q / qd` through the host forms - the
device forms' own definition.  Every comparison is byte equality: the feature moves data and calls shc_engine_step_k, which has its own tests.

Fleet and inputs are those of tests/test_gpu_fleet_device_io.py, by import: 46 robots in three bins (23 hexapods, 14 octopods, 9 mixed-DOF), every
part ends in a partly filled wavefront, both per-leg directions are padded to 8 x 5 with SENTINEL in the padding, quaternions are not normalised."""
import ctypes as C
import functools

import numpy as np
import pytest

from syropod_highlevel_controller_amd.engine import (SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, SHC_ERR_UNSUPPORTED, SHC_OK, FleetInputs, ShcError, device_count)
from syropod_highlevel_controller_amd.fleet import MixedFleet
from test_gpu_fleet_device_io import (DOF, HEX, LEGS, MD, MIX, ML, MORPH, N, OCT, SENTINEL, host_set, input_set, joint_bytes, make, robot_records, to_device,
                                      views)
from test_gpu_resident import config3_params

pytestmark = pytest.mark.gpu

GROUPS = ("linear_xy", "angular", "imu_orientation_wxyz", "imu_angular_velocity", "tip_force", "joint_effort")
K1 = 5   # case 1's K


def k_rows(seed, K, names=GROUPS):
    """K rows of every K-deep input: row k is input_set(100 * seed + k) without its pose members."""
    sets = [input_set(100 * seed + k) for k in range(K)]
    return {name: np.ascontiguousarray(np.stack([s[name] for s in sets])) for name in names}


def row(rows, k):
    return {name: v[k] for name, v in rows.items()}


def warm(fleet):
    """Every input once - the pose inputs too: they are held through everything that follows - and 20 cycles of walking."""
    host_set(fleet, input_set(90))
    fleet.step(20)


def twin_loop(b, rows, K):
    """The definition, on the host route: [(q bytes, qd bytes)] of the K cycles."""
    out = []
    for k in range(K):
        host_set(b, row(rows, k))
        b.step(1)
        q, qd = b.joints()
        out.append((q.tobytes(), qd.tobytes()))
    return out


def ring_buffers(fleet, count, which=("q", "qd")):
    """Buffers for MixedFleet.step_k_joints, every byte 0xAB beforehand: (typed views, raw bytes)."""
    import torch
    shape = (count, fleet.n, fleet.max_legs, fleet.max_dof)
    raw = {k: torch.full((int(np.prod(shape)) * 8,), 0xAB, dtype=torch.uint8, device="cuda") for k in which}
    torch.cuda.synchronize()
    return {k: v.view(torch.float64).view(shape) for k, v in raw.items()}, raw


def per_cycle(fleet, raw, count):
    size = fleet.n * fleet.max_legs * fleet.max_dof * 8
    host = {k: v.cpu().numpy().tobytes() for k, v in raw.items()}
    return [tuple(host[k][c * size:(c + 1) * size] for k in ("q", "qd")) for c in range(count)]


def read_cycles(fleet, first, count):
    out, raw = ring_buffers(fleet, count)
    fleet.step_k_joints(first, count, **out)
    fleet.synchronize()
    return per_cycle(fleet, raw, count)


def assert_records(got, want, what):
    for i in range(N):
        assert got[i] == want[i], f"{what}: robot {i} (bin {MORPH[i]}) holds other records than the twin's"
    sentinel = np.float64(SENTINEL).tobytes()
    assert not any(sentinel in part for rec in got for part in rec), f"{what}: a padding entry of a per-leg input reached the state"


@functools.lru_cache(maxsize=None)
def twin(rough, K):
    """Case 1's twin (and case 2's): computed once, shared by the tests that compare against it, never changed."""
    (b,) = make(1, rough=rough)
    warm(b)
    cycles = twin_loop(b, k_rows(1, K), K)
    records = robot_records(b)
    b.step(7)
    out = {"cycles": cycles, "records": records, "records7": robot_records(b), "joints7": joint_bytes(b)}
    b.close()
    return out


def assert_matches_twin(a, t, K):
    """Everything the definition names, in the order the twin read it: every cycle's q / qd, the records, and - the last row is the held input -
    the records and joints seven held cycles later."""
    got = read_cycles(a, 0, K)
    for k in range(K):
        assert got[k][0] == t["cycles"][k][0], f"q of cycle {k} differs from the twin's"
        assert got[k][1] == t["cycles"][k][1], f"qd of cycle {k} differs from the twin's"
    assert_records(robot_records(a), t["records"], f"after step_k({K})")
    a.step(7)
    assert_records(robot_records(a), t["records7"], "7 cycles after step_k")
    assert joint_bytes(a) == t["joints7"]
    q = np.frombuffer(got[0][0]).reshape(N, ML, MD)
    assert np.isnan(q[HEX[0], 6:]).all() and np.isnan(q[HEX[0], :6, 3:]).all() and np.isnan(q[MIX[0], 6:]).all() and np.isfinite(q[OCT]).all()


def definition_case(rough, K):
    a, c = make(2, rough=rough)
    for f in (a, c):
        warm(f)
    rows = k_rows(1, K)
    dev = to_device(rows)
    a.step_k(K, **dev)
    a.synchronize()            # (the K-deep arrays stay untouched until the parts have read them)
    t = twin(rough, K)
    assert_matches_twin(a, t, K)
    # C: row 0 in all K rows.  It must end elsewhere, otherwise the rows after the first were never read and the comparison shows nothing
    same = to_device({name: np.ascontiguousarray(np.repeat(v[:1], K, axis=0)) for name, v in rows.items()})
    c.step_k(K, **same)
    c.synchronize()
    got = read_cycles(c, 0, K)
    assert got[0] == t["cycles"][0]
    assert got[K - 1] != t["cycles"][K - 1], "K times row 0 gives the twin's last cycle: the rows change nothing"
    for f in (a, c):
        f.close()


def test_definition():
    """Case 1: K = 5, all six arrays."""
    definition_case(False, K1)


def test_definition_rough_terrain():
    """Case 2: rough_terrain_mode on every bin, K = 4: touchdown detection on each cycle's fresh tip forces, inside the loop."""
    definition_case(True, 4)


def test_held_groups():
    """Case 3: only the velocity pair is K-deep, the others are held from an earlier set_inputs; then rows = NULL (and the all-NULL struct)."""
    a, b = make()
    for f in (a, b):
        warm(f)
    held = input_set(31)
    a.set_inputs(**to_device(held))
    host_set(b, held)
    K = 4
    rows = k_rows(3, K, ("linear_xy", "angular"))
    dev = to_device(rows)
    a.step_k(K, **dev)
    a.synchronize()
    assert read_cycles(a, 0, K) == twin_loop(b, rows, K)
    assert_records(robot_records(a), robot_records(b), "after a step_k of velocities only")
    assert a.L.shc_fleet_step_k(a.h, 3, None) == SHC_OK
    last = read_cycles(a, 2, 1)
    b.step(3)
    q, qd = b.joints()
    assert last == [(q.tobytes(), qd.tobytes())], "rows = NULL, K = 3: the last cycle is not what step(3) gives"
    a.step_k(2)
    last = read_cycles(a, 1, 1)
    b.step(2)
    q, qd = b.joints()
    assert last == [(q.tobytes(), qd.tobytes())]
    assert_records(robot_records(a), robot_records(b), "after step_k with every input held")
    for f in (a, b):
        f.close()


def test_serial_form_inside_a_fleet():
    """Case 4: SHC_FEAT_STEP_K_SERIAL on the hexapod part: that part runs its K cycles as single launches, the other two their batch kernels."""
    from syropod_highlevel_controller_amd.params import FEAT_DEFAULT, FEAT_STEP_K_SERIAL
    (a,) = make(1)
    warm(a)
    hexapods, ids = views(a)[0]
    assert list(ids) == list(HEX)
    hexapods.set_features(FEAT_DEFAULT | FEAT_STEP_K_SERIAL)
    dev = to_device(k_rows(1, K1))
    a.step_k(K1, **dev)
    a.synchronize()
    assert_matches_twin(a, twin(False, K1), K1)
    a.close()


def test_ranges_and_shapes():
    """Case 5: K = 1; (first, count) = (2, 2) and (K - 1, 1); q alone and qd alone; 0xAB buffers, every byte rewritten, the other buffer untouched."""
    (a,) = make(1)
    warm(a)
    t = twin(False, K1)
    rows = k_rows(1, K1)
    one = to_device({name: np.ascontiguousarray(v[:1]) for name, v in rows.items()})
    a.step_k(1, **one)         # K = 1 with row 0: the twin's cycle 0
    a.synchronize()
    assert read_cycles(a, 0, 1) == t["cycles"][:1]
    rest = to_device({name: np.ascontiguousarray(v[1:]) for name, v in rows.items()})
    a.step_k(K1 - 1, **rest)   # ... and rows 1 .. 4 behind it: cycles 0 .. 3 of this call are the twin's 1 .. 4
    a.synchronize()
    K = K1 - 1
    for first, count in ((2, 2), (K - 1, 1)):
        assert read_cycles(a, first, count) == t["cycles"][1 + first:1 + first + count], (first, count)
        for which in (0, 1):
            out, raw = ring_buffers(a, count)
            a.step_k_joints(first, count, **{("q", "qd")[which]: out[("q", "qd")[which]]})
            a.synchronize()
            got = per_cycle(a, raw, count)
            assert [g[which] for g in got] == [c[which] for c in t["cycles"][1 + first:1 + first + count]], (first, count, which)
            other = raw[("q", "qd")[1 - which]].cpu().numpy().tobytes()
            assert other == b"\xab" * len(other), "a buffer that was not asked for was written"
    out, raw = ring_buffers(a, K)
    a.step_k_joints(q=out["q"], qd=out["qd"])   # count = None: the buffers' own K rows
    a.synchronize()
    assert per_cycle(a, raw, K) == t["cycles"][1:]
    assert_records(robot_records(a), t["records"], "after step_k(1) + step_k(4)")
    a.close()


def test_staging():
    """Case 6: io_nbytes grows at the first call by K x rows x (10 + 3 L + L D) doubles per part, not at a second identical call, grows for a
    larger K, and not for a smaller K afterwards; all four calls give the twin's cycles."""
    a, b = make()
    for f in (a, b):
        warm(f)
    first = input_set(91)
    a.set_inputs(**to_device(first))
    host_set(b, first)
    a.synchronize()
    base = a.io_nbytes
    assert base > 0
    per_cycle_bytes = 8 * sum(len(ids) * (10 + 3 * LEGS[m] + LEGS[m] * DOF[m]) for m, ids in enumerate((HEX, OCT, MIX)))
    sizes = []
    for i, K in enumerate((2, 2, 4, 3)):
        rows = k_rows(60 + i, K)
        dev = to_device(rows)
        a.step_k(K, **dev)
        a.synchronize()
        assert read_cycles(a, 0, K) == twin_loop(b, rows, K), f"call {i} (K = {K})"
        sizes.append(a.io_nbytes)
    assert sizes[0] == base + 2 * per_cycle_bytes
    assert sizes[1] == sizes[0], "a second identical call allocated"
    assert sizes[2] == base + 4 * per_cycle_bytes
    assert sizes[3] == sizes[2], "a call with a smaller K allocated"
    assert_records(robot_records(a), robot_records(b), "after four step_k calls")
    for f in (a, b):
        f.close()


def test_split_launches():
    """Case 7: 40 963 hexapods in one part of its own on the device: 4 097 wavefronts, so the part's launches go out as two halves on two internal
    streams.  Two step_k calls back to back with different rows and no synchronise between them: the second pack overwrites the staging the
    first call's halves read, which only the join orders.  The smallest shape at which a missing join can go wrong."""
    if device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    n, K = 40963, 3
    morph = np.zeros(n, dtype=np.int32)
    a, b = (MixedFleet([config3_params()], morph) for _ in range(2))
    assert (a.max_legs, a.max_dof) == (6, 3)
    assert -(-n // (64 // 6)) == 4097   # ten hexapods per wavefront: one wavefront past the 4 096 from which a part alone on its device steps split
    rng = np.random.default_rng(7)
    calls = [{"linear_xy": rng.uniform(-0.6, 0.6, (K, n, 2)), "angular": rng.uniform(-0.8, 0.8, (K, n)),
              "tip_force": np.ascontiguousarray(np.stack([rng.normal(0, 1, (K, n, 6)), rng.normal(0, 1, (K, n, 6)), rng.uniform(0, 15, (K, n, 6))], axis=3)),
              "joint_effort": rng.normal(0, 2, (K, n, 6, 3))} for _ in range(2)]
    dev = [to_device(x) for x in calls]
    out, raw = ring_buffers(a, K)
    a.step(2)
    a.step_k(K, **dev[0])
    a.step_k(K, **dev[1])
    a.step_k_joints(q=out["q"], qd=out["qd"])
    a.synchronize()
    b.step(2)
    twin_loop(b, calls[0], K)
    want = twin_loop(b, calls[1], K)
    got = per_cycle(a, raw, K)
    for k in range(K):
        assert got[k] == want[k], f"cycle {k} of the second call differs from the twin's"
    assert joint_bytes(a) == joint_bytes(b)
    for f in (a, b):
        f.close()


def test_ordering_calls():
    """Case 8.  As the device I/O's own test of the ordering calls this cannot prove the ordering at this size; it proves that the calls compose
    and lose nothing: the rows are produced by torch kernels on a side stream s, then order_after(s), step_k, step_k_joints, order_before(s), a
    consumer on s - which also overwrites the K-deep arrays, free by then - and ONE host synchronise at the end."""
    import torch
    (a,) = make(1)
    warm(a)
    a.synchronize()
    reversed_rows = to_device({name: np.ascontiguousarray(v[::-1]) for name, v in k_rows(1, K1).items()})
    out, raw = ring_buffers(a, K1)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        made = {name: v.flip(0).contiguous() for name, v in reversed_rows.items()}   # (exact: the rows of case 1, written on s)
    a.order_after(s)
    a.step_k(K1, **made)
    a.step_k_joints(q=out["q"], qd=out["qd"])
    a.order_before(s)
    with torch.cuda.stream(s):
        copy = {k: v.clone() for k, v in raw.items()}
        for v in made.values():
            v.zero_()
    s.synchronize()
    t = twin(False, K1)
    assert per_cycle(a, copy, K1) == t["cycles"]
    assert_matches_twin(a, t, K1)
    a.close()


def test_refusals_change_nothing():
    """Case 9: the records of every robot and the bytes of the output buffers before and after each refusal."""
    import torch
    (a,) = make(1)
    L = a.L
    warm(a)
    dev = to_device(k_rows(9, 3))
    pose = torch.zeros((3, N, 3), dtype=torch.float64, device="cuda")
    out, raw = ring_buffers(a, 3)
    torch.cuda.synchronize()
    hexapods = views(a)[0][0]
    hexapods.resident_begin(ring_depth=4, max_cycles=100)
    hexapods.resident_end()    # (whatever entering and leaving resident mode itself leaves in the records is in `before`)
    before = robot_records(a)

    def rows_of(**members):
        st = FleetInputs()
        for name, v in members.items():
            setattr(st, name, v.data_ptr())
        return st

    def untouched(what):
        a.synchronize()
        assert robot_records(a) == before, f"{what}: a refused call changed a robot"
        assert all(v.cpu().numpy().tobytes() == b"\xab" * v.numel() for v in raw.values()), f"{what}: a refused call wrote to a buffer"

    step_k = lambda K, st: L.shc_fleet_step_k(a.h, K, C.byref(st))
    joints = lambda first, count, q, qd: L.shc_fleet_get_step_k_joints_device(a.h, first, count, q, qd)
    q, qd = out["q"].data_ptr(), out["qd"].data_ptr()
    everything = rows_of(**dev)
    assert joints(0, 1, q, qd) == SHC_ERR_INVALID_ARG                        # a read before any step_k
    with pytest.raises(ShcError):
        a.step_k_joints(0, 1, q=out["q"][:1])
    untouched("a read before any step_k")
    assert step_k(0, everything) == SHC_ERR_INVALID_ARG and step_k(4097, everything) == SHC_ERR_INVALID_ARG
    assert step_k(-1, everything) == SHC_ERR_INVALID_ARG
    untouched("K = 0 / 4097")
    assert step_k(3, rows_of(linear_xy=dev["linear_xy"])) == SHC_ERR_INVALID_ARG       # half a pair
    assert step_k(3, rows_of(angular=dev["angular"])) == SHC_ERR_INVALID_ARG
    assert step_k(3, rows_of(imu_orientation_wxyz=dev["imu_orientation_wxyz"])) == SHC_ERR_INVALID_ARG
    assert step_k(3, rows_of(imu_angular_velocity=dev["imu_angular_velocity"])) == SHC_ERR_INVALID_ARG
    untouched("half a pair")
    assert step_k(3, rows_of(pose_translation_velocity=pose, **dev)) == SHC_ERR_UNSUPPORTED
    assert step_k(3, rows_of(pose_rotation_velocity=pose)) == SHC_ERR_UNSUPPORTED
    with pytest.raises(ShcError, match="pose"):
        a.step_k(3, pose_rotation_velocity=pose)
    untouched("a pose member")
    with pytest.raises(ValueError, match=r"\(3, 46, 8, 3\)"):
        a.step_k(3, tip_force=dev["tip_force"][:, :, :6])
    with pytest.raises(ValueError):
        a.step_k(2, **dev)                                                   # K rows are expected, three are given
    with pytest.raises(TypeError):
        a.step_k(3, velocity=dev["angular"])
    untouched("shapes and names")
    # a part in resident mode: both calls are busy
    hexapods.resident_begin(ring_depth=4, max_cycles=100)
    try:
        assert step_k(3, everything) == SHC_ERR_BUSY
        assert joints(0, 1, q, qd) == SHC_ERR_BUSY
    finally:
        hexapods.resident_end()
    untouched("a part in resident mode")
    # ... and after a call that was accepted: the reads that are refused
    assert step_k(3, everything) == SHC_OK
    a.synchronize()
    before = robot_records(a)
    assert joints(0, 3, None, None) == SHC_ERR_INVALID_ARG                   # both outputs NULL
    with pytest.raises(ShcError):
        a.step_k_joints(0, 3)
    for first, count in ((2, 2), (3, 1), (0, 4), (-1, 1), (0, 0), (1, -1)):  # a range past K
        assert joints(first, count, q, qd) == SHC_ERR_INVALID_ARG, (first, count)
    assert joints(0, 3, q + 4, None) == SHC_ERR_INVALID_ARG and joints(0, 3, None, qd + 4) == SHC_ERR_INVALID_ARG   # misaligned
    with pytest.raises(ValueError):
        a.step_k_joints(0, 2, q=out["q"])                                    # two cycles are expected, the buffer has three
    untouched("refused reads")
    # the handle still works
    assert joints(0, 3, q, qd) == SHC_OK
    a.synchronize()
    got = per_cycle(a, raw, 3)
    assert got[2] == tuple(x.tobytes() for x in a.joints())
    a.close()


def test_a_fleet_over_two_devices_is_refused():
    """Case 9, last item: both calls answer SHC_ERR_UNSUPPORTED, as the other device entry points."""
    if device_count() < 2:
        pytest.skip("one device visible: a fleet over two devices cannot be built")
    (a,) = make(1, devices=(0, 1))
    dev = to_device(k_rows(9, 2, ("linear_xy", "angular")))
    out, raw = ring_buffers(a, 2, ("q",))
    st = FleetInputs()
    st.linear_xy, st.angular = dev["linear_xy"].data_ptr(), dev["angular"].data_ptr()
    before = robot_records(a)
    assert a.L.shc_fleet_step_k(a.h, 2, C.byref(st)) == SHC_ERR_UNSUPPORTED
    assert a.L.shc_fleet_step_k(a.h, 2, None) == SHC_ERR_UNSUPPORTED
    assert a.L.shc_fleet_get_step_k_joints_device(a.h, 0, 1, out["q"].data_ptr(), None) == SHC_ERR_UNSUPPORTED
    assert a.io_nbytes == 0
    assert robot_records(a) == before
    assert raw["q"].cpu().numpy().tobytes() == b"\xab" * raw["q"].numel()
    a.close()
