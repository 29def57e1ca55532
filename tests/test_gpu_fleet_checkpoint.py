"""GPU (-m gpu): fleet checkpoints (shc_fleet_checkpoint_*, shc_fleet_restore_instances, shc_fleet_scan_and_restore) against their definition, the
engine route part by part: after a fleet restore, the shc_engine_get_state / get_aux_state records of every robot's slot in its part are what the
captured records say, and the fleet walks on bit for bit like a twin fleet that received the same records through shc_engine_set_state /
set_aux_state on its parts.  Every comparison is byte equality: the feature moves state, it computes nothing.

Fleet: 23 hexapods (6x3; ten per wavefront) and 14 octopods (8x5; eight per wavefront) interleaved, so that both parts end in a partly filled
wavefront and the caller's order differs from both parts' orders; admittance control and IMU posing on (the feature set of
tests/test_gpu_checkpoint.py), a velocity command of its own per robot and tip forces on every leg."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (HEALTH_NONFINITE, SHC_ERR_INVALID_ARG, SHC_ERR_UNSUPPORTED, SHC_OK, BatchEngine, ShcError,
                                                     device_count)
from syropod_highlevel_controller_amd.fleet import MixedFleet
from test_gpu_checkpoint import host_restore, per_robot, records, with_config3_features
from test_gpu_resident import config3_params, state_bytes
from test_gpu_teacher_forced import as_np

pytestmark = pytest.mark.gpu

N = 37
MORPH = np.array([1 if (i % 5 in (1, 3) and i != 36) else 0 for i in range(N)], dtype=np.int32)
HEX, OCT = np.flatnonzero(MORPH == 0), np.flatnonzero(MORPH == 1)   # 23 and 14 caller ids, ascending: the parts' own orders
assert len(HEX) == 23 and len(OCT) == 14


def make(count=2, devices=(0,)):
    if device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    morphs = [config3_params(), with_config3_features(synthetic_octopod_params("ripple", 5, 8))]
    return [MixedFleet(morphs, MORPH, devices) for _ in range(count)]


def drive(fleets, seed, cycles):
    """A velocity command per robot and tip forces on every leg (a different set per seed), then `cycles` cycles, on every fleet alike."""
    rng = np.random.default_rng(seed)
    lin, ang = rng.uniform(-0.6, 0.6, (N, 2)), rng.uniform(-0.8, 0.8, N)
    force = np.ascontiguousarray(np.stack([rng.normal(0, 1, (N, 8)), rng.normal(0, 1, (N, 8)), rng.uniform(0, 15, (N, 8))], axis=2))
    for f in fleets:
        f.set_velocity(lin, ang)
        assert f.L.shc_fleet_set_tip_force(f.h, force.ctypes.data_as(C.c_void_p)) == SHC_OK
        f.step(cycles)


def views(fleet):
    """[(non-owning engine view, caller ids)] of the fleet's parts."""
    return [(BatchEngine.view(handle, fleet.params[m], len(ids)), ids) for handle, m, _, ids in fleet.parts()]


def robot_records(fleet):
    """(state record bytes, auxiliary blob bytes) of every robot, read through its part's engine, in the caller's order."""
    out = [None] * N
    for view, ids in views(fleet):
        s, x = per_robot(state_bytes(view), len(ids)), per_robot(view.get_aux_state(), len(ids))
        for j, i in enumerate(ids):
            out[i] = (s[j], x[j])
    assert all(r is not None for r in out)
    return out


def part_records(fleet):
    """What the host route needs: the (state array, aux blobs) pair of every part."""
    return [records(view) for view, _ in views(fleet)]


def host_route(fleet, recs, source):
    """The definition: the caller's map translated into each part's own ids, then set_state / set_aux_state on the part's engine (host_restore of
    tests/test_gpu_checkpoint.py); a part the map does not name is not touched."""
    for (view, ids), rec in zip(views(fleet), recs):
        local_of = {int(i): j for j, i in enumerate(ids)}
        local = np.array([local_of[int(source[i])] if source[i] >= 0 else -1 for i in ids], dtype=np.int64)
        if (local >= 0).any():
            host_restore(view, rec, local)


def joint_bytes(fleet):
    q, qd = fleet.joints()
    return q.tobytes() + qd.tobytes()


def expect_records(after, source, captured, before, what):
    for i in range(N):
        want = captured[int(source[i])] if source[i] >= 0 else before[i]
        assert after[i] == want, f"{what}: robot {i} (source {int(source[i])}) does not hold the expected records"
    assert any(captured[i] != before[i] for i in range(N)), "the cycles between capture and restore did not move the state"


def capture_at_30_walk_to_70(a, b):
    """Common history of a fleet and its twin: 30 cycles, checkpoint on A (records read on both), 40 cycles on other commands."""
    drive((a, b), 1, 30)
    ck = a.checkpoint()
    captured, recs_b = robot_records(a), part_records(b)
    assert captured == robot_records(b)
    drive((a, b), 2, 40)
    return ck, captured, recs_b


def restore_and_walk_on(a, b, ck, captured, recs_b, source):
    before = robot_records(a)
    assert before == robot_records(b)
    a.restore(ck, source)
    host_route(b, recs_b, source)
    after = robot_records(a)
    expect_records(after, source, captured, before, "right after the restore")
    assert after == robot_records(b), "the fleet restore and the host route on the twin's parts left different records"
    drive((a, b), 3, 40)
    assert joint_bytes(a) == joint_bytes(b), "40 cycles after the restore the fleet and its twin differ"
    assert robot_records(a) == robot_records(b)


def subset_map():
    """Both morphologies: the first and the last robot of each part and robots of the partly filled wavefronts (hexapods 20.., octopods 8..)."""
    m = np.full(N, -1, dtype=np.int64)
    for i in [HEX[0], HEX[9], HEX[10], HEX[20], HEX[22], OCT[0], OCT[7], OCT[8], OCT[13]]:
        m[i] = i
    return m


def clone_map():
    """One hexapod onto several across the wavefront boundaries, the octopods shifted by five (sources across the boundary at eight); i != source[i]."""
    m = np.full(N, -1, dtype=np.int64)
    for k in (3, 9, 10, 15, 22):
        m[HEX[k]] = HEX[0]
    m[HEX[1]] = HEX[21]
    for k in range(len(OCT)):
        m[OCT[k]] = OCT[(k + 5) % len(OCT)]
    assert all(m[i] != i for i in range(N))
    return m


def test_reset_a_subset():
    """Case 1."""
    a, b = make()
    ck, captured, recs_b = capture_at_30_walk_to_70(a, b)
    assert ck.nbytes > 0
    restore_and_walk_on(a, b, ck, captured, recs_b, subset_map())
    ck.close()
    ck.close()
    for f in (a, b):
        f.close()


def test_clone():
    """Case 2."""
    a, b = make()
    ck, captured, recs_b = capture_at_30_walk_to_70(a, b)
    restore_and_walk_on(a, b, ck, captured, recs_b, clone_map())
    for f in (a, b):
        f.close()


def test_device_map_equals_host_map():
    """Case 3: the same map as a torch device tensor on one fleet and as a numpy array on its twin; then a device map whose entries >= n, < 0 and of the
    other morphology leave exactly their destinations untouched."""
    import torch
    a, b = make()
    drive((a, b), 1, 30)
    cka, ckb = a.checkpoint(), b.checkpoint()
    captured = robot_records(a)
    assert captured == robot_records(b)
    drive((a, b), 2, 40)
    m = clone_map()
    m[HEX[5]], m[OCT[2]] = HEX[5], -1
    t = torch.from_numpy(m).cuda()
    torch.cuda.synchronize()   # the parts run on streams of their own: the map is complete before the call
    before = robot_records(a)
    a.restore(cka, t)
    b.restore(ckb, m)
    after = robot_records(a)
    expect_records(after, m, captured, before, "device map")
    assert after == robot_records(b)
    drive((a, b), 3, 20)
    assert joint_bytes(a) == joint_bytes(b) and robot_records(a) == robot_records(b)
    # entries that name nobody a robot could be restored from
    bad = np.full(N, -1, dtype=np.int64)
    bad[HEX[0]], bad[HEX[22]], bad[OCT[0]] = N, N + 12345, 2 ** 40          # >= n
    bad[HEX[4]], bad[OCT[13]] = -5, -2 ** 40                                # < 0
    bad[HEX[10]], bad[HEX[21]], bad[OCT[8]], bad[OCT[12]] = OCT[0], OCT[13], HEX[0], HEX[22]   # the other morphology
    bad[HEX[2]], bad[OCT[1]] = HEX[19], OCT[1]                              # ... next to two entries that do restore
    effective = np.full(N, -1, dtype=np.int64)
    effective[HEX[2]], effective[OCT[1]] = HEX[19], OCT[1]
    cka.update()
    captured = robot_records(a)
    drive((a,), 4, 10)
    before = robot_records(a)
    t = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    a.restore(cka, t)
    expect_records(robot_records(a), effective, captured, before, "device map with entries that name nobody")
    with pytest.raises(ValueError):
        a.restore(cka, torch.zeros(N - 1, dtype=torch.int64, device="cuda"))
    for f in (a, b):
        f.close()


def refreshed_records(fleet):
    """robot_records behind a scan.  The auxiliary blob carries the LegPoser tip position, which is an output the engine derives from the stored state
    when a getter or a scan asks (not in every cycle): the blob of a robot is a function of its state only once that pass has run on the state."""
    fleet.scan_health()
    return robot_records(fleet)


def test_scan_and_restore():
    """Case 4: a NaN joint angle planted in three hexapods and two octopods, the last slot of each part among them.  Every record is read behind a
    scan (refreshed_records): scan_and_restore itself refreshes the derived tips, as shc_engine_scan_health does."""
    (a,) = make(1)
    drive((a,), 1, 30)
    ck = a.checkpoint()
    captured = refreshed_records(a)
    drive((a,), 2, 40)
    sick = {int(HEX[0]), int(HEX[11]), int(HEX[22]), int(OCT[5]), int(OCT[13])}
    for view, ids in views(a):
        states = view.get_state()
        s = as_np(states)
        for j, i in enumerate(ids):
            if int(i) in sick:
                s["leg"]["joint_position"][j, 1, 0] = np.nan
        view.set_state(states)
    pre = a.scan_health(select=HEALTH_NONFINITE)
    before = robot_records(a)
    n_restored, rec = a.scan_and_restore(ck, HEALTH_NONFINITE, health=True)
    assert n_restored == 5
    assert rec.tobytes() == pre.tobytes(), "the returned records are the records before the restore"
    assert {i for i in range(N) if rec["flags"][i] & HEALTH_NONFINITE} == sick
    source = np.array([i if i in sick else -1 for i in range(N)], dtype=np.int64)
    after = refreshed_records(a)
    expect_records(after, source, captured, before, "scan and restore")
    assert a.scan_and_restore(ck, HEALTH_NONFINITE) == 0   # nobody is unhealthy any more
    assert robot_records(a) == after
    drive((a,), 3, 30)
    q, qd = a.joints()
    for x in (q, qd):
        assert np.isfinite(x[HEX][:, :6, :3]).all() and np.isfinite(x[OCT]).all()
    # criteria = NULL selects nobody: a scan and nothing else
    before = refreshed_records(a)
    n_sel = C.c_int64(-1)
    health = np.zeros(N, dtype=rec.dtype)
    assert a.L.shc_fleet_scan_and_restore(a.h, ck.h, None, health.ctypes.data_as(C.c_void_p), C.byref(n_sel)) == SHC_OK
    assert n_sel.value == 0 and health.tobytes() == a.scan_health(0, -np.inf, np.inf).tobytes()
    assert a.L.shc_fleet_scan_and_restore(a.h, ck.h, None, None, None) == SHC_OK
    assert a.scan_and_restore(ck, 0) == 0
    assert robot_records(a) == before
    a.close()


def test_refusals_change_nothing():
    """Case 5."""
    a, b = make()
    L = a.L
    restore = lambda f, ck, src=None, dev=0: L.shc_fleet_restore_instances(f.h, ck.h, None if src is None else src.ctypes.data_as(C.c_void_p), dev)
    drive((a, b), 1, 30)
    ck, ckb = a.checkpoint(), b.checkpoint()
    drive((a,), 2, 10)

    def refused(code, *args):
        before = robot_records(a)
        assert restore(*args) == code, L.shc_last_error()
        assert robot_records(a) == before

    m = subset_map()
    m[HEX[2]] = OCT[1]
    refused(SHC_ERR_INVALID_ARG, a, ck, m)                                # a source of another morphology
    m = subset_map()
    m[OCT[3]] = N
    refused(SHC_ERR_INVALID_ARG, a, ck, m)                                # an entry >= n
    with pytest.raises(ShcError):
        a.restore(ck, m)
    with pytest.raises(ValueError):
        a.restore(ck, np.arange(N - 1))
    refused(SHC_ERR_INVALID_ARG, a, ckb)                                  # another fleet's checkpoint
    refused(SHC_ERR_INVALID_ARG, a, ckb, subset_map())
    assert L.shc_fleet_checkpoint_update(a.h, ckb.h) == SHC_ERR_INVALID_ARG
    assert L.shc_fleet_scan_and_restore(a.h, ckb.h, None, None, None) == SHC_ERR_INVALID_ARG
    # a gait change on the hexapods' part: the octopods' restore is refused with it, and neither part has moved
    (hexapods, _), _ = views(a)
    a.set_velocity(np.zeros((N, 2)), np.zeros(N))
    for _ in range(40):
        a.step(25)
        if hexapods.change_gait(with_config3_features(default_hexapod_params("tripod"))) == 0:
            break
    else:
        pytest.fail("the robots did not stop")
    only_octopods = np.full(N, -1, dtype=np.int64)
    only_octopods[OCT] = OCT
    refused(SHC_ERR_UNSUPPORTED, a, ck, only_octopods)
    before = robot_records(a)
    assert L.shc_fleet_scan_and_restore(a.h, ck.h, None, None, None) == SHC_ERR_UNSUPPORTED
    assert robot_records(a) == before
    a.step(1)
    ck.update()
    captured = robot_records(a)
    drive((a,), 3, 5)
    before = robot_records(a)
    assert restore(a, ck, only_octopods) == SHC_OK
    expect_records(robot_records(a), only_octopods, captured, before, "after the update")
    # the fleet first, its checkpoint second
    assert L.shc_fleet_destroy(a.h) == SHC_OK
    a.h = None
    assert ck.nbytes == 0
    assert L.shc_fleet_checkpoint_update(b.h, ck.h) == SHC_ERR_INVALID_ARG
    assert L.shc_fleet_restore_instances(b.h, ck.h, None, 0) == SHC_ERR_INVALID_ARG
    ck.close()
    assert ck.h is None
    with b.checkpoint() as scoped:
        assert scoped.nbytes > 0
    assert scoped.h is None
    held = b.checkpoint()
    b.close()                                                             # closes its checkpoints with it
    assert held.h is None and ckb.h is None


def test_cross_part_source():
    """Case 6: two shards of every morphology on device 0 (shc_fleet_create takes a repeated device id): hexapods 12 + 11, octopods 7 + 7."""
    import torch
    (a,) = make(1, devices=(0, 0))
    parts = a.parts()
    assert [len(ids) for _, _, _, ids in parts] == [12, 11, 7, 7] and [m for _, m, _, _ in parts] == [0, 0, 1, 1]
    drive((a,), 1, 30)
    ck = a.checkpoint()
    captured = robot_records(a)
    drive((a,), 2, 20)
    m = np.full(N, -1, dtype=np.int64)
    m[HEX[0]], m[HEX[13]], m[OCT[2]] = HEX[20], HEX[14], OCT[6]   # HEX[0] <- the other shard; the other two stay inside their shards
    before = robot_records(a)
    assert a.L.shc_fleet_restore_instances(a.h, ck.h, m.ctypes.data_as(C.c_void_p), 0) == SHC_ERR_UNSUPPORTED
    assert robot_records(a) == before
    t = torch.from_numpy(m).cuda()
    torch.cuda.synchronize()
    a.restore(ck, t)                                              # the device form leaves that destination alone
    effective = m.copy()
    effective[HEX[0]] = -1
    expect_records(robot_records(a), effective, captured, before, "device map with a source in the other shard")
    a.close()


def test_reading_does_not_disturb():
    """Case 7."""
    a, b = make()
    drive((a, b), 1, 30)
    ck = a.checkpoint()
    a.step(3)
    b.step(3)
    ck.update()
    drive((a, b), 2, 40)
    assert joint_bytes(a) == joint_bytes(b)
    for f in (a, b):
        f.close()
