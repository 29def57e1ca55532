"""Device checkpoints (shc_engine_checkpoint_* / shc_engine_restore_instances) against their definition, the host route.

Method of every case: engine A and a twin engine B run the same deterministic history.  At capture time A makes a device checkpoint and the
test reads B's get_state / get_aux_state records.  Both go on differently from there (other commands for 40 cycles).  A restores through
the new call, B restores the same rows through set_state / set_aux_state.  Both then get the same fresh inputs and 30 more cycles.
Required: the state records, the auxiliary blobs and joints() right after the restore, and q / qd and the state records after the 30 cycles,
are equal BYTE FOR BYTE between A and B - a restore is a copy, so there is no tolerance.

Shapes: the smallest with three or more wavefronts and a partly filled last one (10 hexapods, 8 octopods, 16 quadrupeds per wavefront)."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, SHC_ERR_UNSUPPORTED, SHC_OK, ShcError, generate_tables
from syropod_highlevel_controller_amd.params import PARAM_STEP_FREQUENCY, PARAM_SWING_HEIGHT, ExternalTarget, InstanceState
from test_gpu_resident import Engine, config3_params, state_bytes  # noqa: F401  (Engine: the module fixture that refuses to run without a device)

pytestmark = pytest.mark.gpu
WAITING = -2


def with_config3_features(p):
    p.admittance_control, p.imu_posing = 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    return p


MORPHOLOGIES = {"6x3": (config3_params, 37), "8x5": (lambda: with_config3_features(synthetic_octopod_params("ripple", 5, 8)), 21),
                "4x4": (lambda: with_config3_features(synthetic_octopod_params("amble", 4, 4)), 35),
                "mixed": (lambda: with_config3_features(synthetic_mixed_dof_params("ripple")), 23)}
_tables = {}


def make(Engine, morph, count=2):
    """`count` engines of one morphology on the same tables (the host init chain runs once per morphology)."""
    build, n = MORPHOLOGIES[morph]
    p = build()
    if morph not in _tables:
        _tables[morph] = generate_tables(p)
    return [Engine(p, n, tables=_tables[morph]) for _ in range(count)], p, n


def inputs(p, n, seed):
    """Velocity, IMU and tip-force inputs: a different set per seed."""
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(seed)
    e = np.stack([rng.uniform(-0.15, 0.15, n), rng.uniform(-0.15, 0.15, n), rng.uniform(-3, 3, n)], axis=1)
    q = R.from_euler("xyz", e).as_quat()
    L = p.leg_count
    return {"lin": rng.uniform(-0.7, 0.7, (n, 2)), "ang": rng.uniform(-1, 1, n), "imu_q": np.stack([q[:, 3], q[:, 0], q[:, 1], q[:, 2]], axis=1),
            "gyro": rng.normal(0, 0.05, (n, 3)), "force": np.stack([rng.normal(0, 1, (n, L)), rng.normal(0, 1, (n, L)), rng.uniform(0, 20, (n, L))], axis=2)}


def drive(e, inp, cycles):
    e.set_velocity(inp["lin"], inp["ang"])
    e.set_imu(inp["imu_q"], inp["gyro"])
    e.set_tip_force(inp["force"])
    e.step(cycles)


def records(e):
    return e.get_state(), e.get_aux_state()


def joint_bytes(e):
    q, qd = e.joints()
    return q.tobytes() + qd.tobytes()


def host_restore(b, rec, source):
    """The definition: rows source[i] of the records read at capture time, written to instances i with set_state / set_aux_state - one call per
    run of consecutive destinations (a map without negative entries is one call over the whole batch)."""
    states, aux = rec
    n, per = b.n, len(aux) // b.n
    source = np.arange(n) if source is None else np.asarray(source)
    i = 0
    while i < n:
        if not 0 <= source[i] < n:
            i += 1
            continue
        j = i
        while j < n and 0 <= source[j] < n:
            j += 1
        rows = (InstanceState * (j - i))(*[states[int(s)] for s in source[i:j]])
        b.set_state(rows, first=i)
        b.set_aux_state(b"".join(aux[int(s) * per:(int(s) + 1) * per] for s in source[i:j]), first=i)
        i = j


def same(a, b, what):
    assert state_bytes(a) == state_bytes(b), f"{what}: state records differ"
    assert a.get_aux_state() == b.get_aux_state(), f"{what}: auxiliary blobs differ"
    assert joint_bytes(a) == joint_bytes(b), f"{what}: joints differ"


def restore_and_compare(a, b, ck, rec, source, p, n, a_source="host"):
    """A restores from the device checkpoint (a_source: the map as a host array, or as given), B by the host route; compare right after and after
    30 more cycles on the same fresh inputs."""
    a.restore(ck, source if a_source == "host" or source is None else a_source)
    host_restore(b, rec, source)
    same(a, b, "right after the restore")
    fresh = inputs(p, n, 99)
    for e in (a, b):
        drive(e, fresh, 30)
    same(a, b, "30 cycles after the restore")


def capture_then_diverge(a, b, p, n, others=()):
    """Common history, capture (checkpoint on A, records from B), then 40 cycles on other commands for every engine."""
    first = inputs(p, n, 1)
    for e in (a, b, *others):
        drive(e, first, 60)
    ck, rec = a.checkpoint(), records(b)
    other = inputs(p, n, 2)
    for e in (a, b, *others):
        drive(e, other, 40)
    return ck, rec


def per_robot(blob, n):
    k = len(blob) // n
    return [blob[i * k:(i + 1) * k] for i in range(n)]


@pytest.mark.parametrize("morph", ["6x3", "8x5", "4x4", "mixed"])
def test_identity_restore_of_everything(Engine, morph):
    """Case 1: config 3's features (admittance + IMU posing + tip force); the velocity / IMU / tip-force inputs change between capture and restore, and the
    restored robots keep the new ones (B's host route does not touch them either, and both walk on identically)."""
    (a, b), p, n = make(Engine, morph)
    ck, rec = capture_then_diverge(a, b, p, n)
    before = state_bytes(a)
    assert ck.nbytes > 0
    restore_and_compare(a, b, ck, rec, None, p, n)
    assert before != bytes(memoryview(rec[0]).cast("B"))   # (the 40 cycles did move the state away from the capture)
    ck.close()
    ck.close()


def sparse_map(n):
    """-1 except one robot of the first group, one of the partly filled last group and a whole wavefront (10 hexapods per wavefront)."""
    m = np.full(n, -1, dtype=np.int64)
    for i in [3, n - 2] + list(range(10, 20)):
        m[i] = i
    return m


def test_sparse_reset_leaves_the_others_alone(Engine):
    """Case 2: untouched robots are byte-identical to a third engine that never restored (it re-injects its own state at that point, so that it carries the
    same engine-wide "a state was injected" facts), right after and 30 cycles later."""
    (a, b, c), p, n = make(Engine, "6x3", 3)
    ck, rec = capture_then_diverge(a, b, p, n, others=(c,))
    m = sparse_map(n)
    c.set_state(c.get_state())
    c.set_aux_state(c.get_aux_state())
    a.restore(ck, m)
    host_restore(b, rec, m)
    same(a, b, "right after the restore")
    captured = per_robot(bytes(memoryview(rec[0]).cast("B")), n)
    sa, sc, xa, xc = per_robot(state_bytes(a), n), per_robot(state_bytes(c), n), per_robot(a.get_aux_state(), n), per_robot(c.get_aux_state(), n)
    for i in range(n):
        if m[i] < 0:
            assert sa[i] == sc[i] and xa[i] == xc[i], f"robot {i} was not restored but changed"
        else:
            assert sa[i] == captured[i] and sa[i] != sc[i], f"robot {i} was not reset to its captured state"
    fresh = inputs(p, n, 99)
    for e in (a, b, c):
        drive(e, fresh, 30)
    same(a, b, "30 cycles after the restore")
    qa, qc = a.joints()[0], c.joints()[0]
    assert all(qa[i].tobytes() == qc[i].tobytes() for i in range(n) if m[i] < 0)


def clone_map(kind, n):
    if kind == "shifted":       # sources across wavefront boundaries
        return (np.arange(n, dtype=np.int64) + 13) % n
    if kind == "reversed":
        return np.arange(n, dtype=np.int64)[::-1].copy()
    return np.full(n, 17, dtype=np.int64)   # one source broadcast to every robot


@pytest.mark.parametrize("kind", ["shifted", "reversed", "broadcast"])
@pytest.mark.parametrize("morph", ["6x3", "8x5"])
def test_clone(Engine, morph, kind):
    """Case 3."""
    (a, b), p, n = make(Engine, morph)
    ck, rec = capture_then_diverge(a, b, p, n)
    restore_and_compare(a, b, ck, rec, clone_map(kind, n), p, n)


@pytest.mark.parametrize("kind", ["sparse", "shifted", "reversed", "broadcast"])
def test_device_map_between_two_steps(Engine, kind):
    """Case 4: the map is a torch int64 tensor built on the engine's stream and the restore is enqueued between two step calls without a host synchronisation;
    the result equals the host-map run.  Entries n and -5 of the device map leave their robots untouched (the host-map run has -1 there)."""
    import torch
    (d, h), p, n = make(Engine, "6x3")
    cd, ch = d.checkpoint(), None
    first, other = inputs(p, n, 1), inputs(p, n, 2)
    for e in (d, h):
        drive(e, first, 60)
    cd.update()
    ch = h.checkpoint()
    for e in (d, h):
        drive(e, other, 39)
    m = sparse_map(n) if kind == "sparse" else clone_map(kind, n)
    m[5], m[n - 1] = -1, -1
    d.step(1)
    t = torch.from_numpy(m).cuda()   # (on the default stream, which is the engine's; nothing waits for it)
    if kind == "sparse":
        done = t >= 0
        t = torch.where(done, torch.arange(n, device="cuda"), torch.full_like(t, -1))   # the mask-to-map idiom
    bad = torch.zeros(n, dtype=torch.int64, device="cuda")
    bad[5], bad[n - 1] = n + 1, 4   # -> entries n and -5
    t = torch.where(bad > 0, torch.where(bad > 4, torch.full_like(t, n), torch.full_like(t, -5)), t).contiguous()
    d.restore(cd, t)
    d.step(1)
    h.step(1)
    h.restore(ch, m)
    h.step(1)
    got = t.cpu().numpy()
    assert got[5] == n and got[n - 1] == -5 and np.array_equal(np.delete(got, [5, n - 1]), np.delete(m, [5, n - 1]))
    same(d, h, "one cycle after the restore")
    fresh = inputs(p, n, 99)
    for e in (d, h):
        drive(e, fresh, 30)
    same(d, h, "30 cycles after the restore")


def toggle_until_done(engines, sel, lin, ang):
    """legStateToggle for the selected leg of each robot (sel < 0: none) on every engine alike, until every selected leg has changed hands."""
    pending = sel >= 0
    lin, ang = lin.copy(), ang.copy()
    for _ in range(3000):
        if not pending.any():
            break
        res = [e.toggle_leg_state(np.where(pending, sel, -1).astype(np.int32)) for e in engines]
        assert all(np.array_equal(res[0], r) for r in res)
        still = res[0] == -1
        if still.any():
            lin[still], ang[still] = 0.0, 0.0
            for e in engines:
                e.set_velocity(lin, ang)
        pending &= ~((res[0] == 1) | (res[0] == 2))
    assert not pending.any()


def manual_params():
    p = default_hexapod_params("tripod")
    p.admittance_control = 1
    return p


def manual_engines(Engine):
    p, n = manual_params(), 37
    if "manual" not in _tables:
        _tables["manual"] = generate_tables(p)
    rng = np.random.default_rng(4)
    lin, ang = rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.5, 0.5, n)
    force = np.abs(rng.normal(0, 2.0, (n, p.leg_count, 3))) + 1.0
    a, b = Engine(p, n, tables=_tables["manual"]), Engine(p, n, tables=_tables["manual"])
    for e in (a, b):
        e.set_velocity(lin, ang)
        e.set_tip_force(force)
        e.step(60)
    sel = np.array([i % p.leg_count if i % 4 else -1 for i in range(n)], dtype=np.int32)   # every fourth robot keeps walking
    return a, b, p, n, lin, ang, force, sel, rng


def manual_finish(a, b, lin, ang, force):
    same(a, b, "right after the restore")
    for e in (a, b):
        e.set_velocity(lin * 0.5, -ang)
        e.set_tip_force(force * 0.8)
        e.step(30)
    same(a, b, "30 cycles after the restore")
    assert np.array_equal(a.leg_manipulation_state(), b.leg_manipulation_state())


def test_records_grown_after_the_capture_are_cleared(Engine):
    """Case 5a: capture before any leg toggle (the engine holds no ManualRobot records), toggle a leg to MANUAL on some robots, restore those robots: their
    records are cleared, as set_aux_state does for a blob without the manual flag."""
    a, b, p, n, lin, ang, force, sel, rng = manual_engines(Engine)
    ck, rec = a.checkpoint(), records(b)
    bytes_before = ck.nbytes
    toggle_until_done((a, b), sel, lin, ang)
    assert (a.leg_manipulation_state()[sel >= 0, sel[sel >= 0]] == 1).all()
    vel = rng.uniform(-0.4, 0.4, (n, 3))
    for e in (a, b):
        e.set_manual_inputs(primary_leg=sel, primary_velocity=vel)
        e.step(7)
    m = np.where(sel >= 0, np.arange(n), -1).astype(np.int64)
    a.restore(ck, m)
    host_restore(b, rec, m)
    assert ck.nbytes == bytes_before
    manual_finish(a, b, lin, ang, force)
    ck.update()   # the engine has grown the manual records since: the checkpoint grows with it, once
    grown = ck.nbytes
    assert grown > bytes_before
    ck.update()
    assert ck.nbytes == grown


def test_manual_leg_in_mid_manipulation(Engine):
    """Case 5b: capture with a manual leg in mid-manipulation, return the leg to walking, restore."""
    a, b, p, n, lin, ang, force, sel, rng = manual_engines(Engine)
    toggle_until_done((a, b), sel, lin, ang)
    vel = rng.uniform(-0.4, 0.4, (n, 3))
    for e in (a, b):
        e.set_manual_inputs(primary_leg=sel, primary_velocity=vel)
        e.step(7)
    ck, rec = a.checkpoint(), records(b)
    for e in (a, b):
        e.set_manual_inputs(primary_leg=sel, primary_velocity=vel * 0.0, primary_position=np.tile([0.25, 0.2, -0.05], (n, 1)))
        e.step(3)
    toggle_until_done((a, b), sel, lin * 0.0, ang * 0.0)
    assert (a.leg_manipulation_state() == 0).all()
    for e in (a, b):
        e.step(10)
    m = np.where(sel >= 0, np.arange(n), -1).astype(np.int64)
    a.restore(ck, m)
    host_restore(b, rec, m)
    assert (a.leg_manipulation_state()[sel >= 0, sel[sel >= 0]] == 1).all()
    manual_finish(a, b, lin, ang, force)


def test_rough_terrain_with_a_pending_external_target(Engine):
    """Case 5c: rough terrain mode, an external target pending on every leg and step planes defined (tip forces above the touchdown threshold have arrived)
    at capture time; the targets are consumed by the swings that follow, then every robot is restored."""
    p, n = default_hexapod_params("tripod"), 37
    p.rough_terrain_mode = 1
    L = p.leg_count
    t = generate_tables(p)
    a, b = Engine(p, n, tables=t), Engine(p, n, tables=t)
    rng = np.random.default_rng(8)
    lin, ang = rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(-0.4, 0.4, n)
    force = np.zeros((n, L, 3))
    force[:, :, 2] = rng.uniform(5.0, 25.0, (n, L))
    tips = None
    for e in (a, b):
        e.set_velocity(lin, ang)
        e.step(50)
        e.set_tip_force(force)
        e.step(15)
        tips = e.leg_state()["walker_tip"].reshape(n, L, 3)
    rows = (ExternalTarget * (n * L))()
    for i in range(n):
        for l in range(L):
            r = rows[i * L + l]
            r.defined = 1
            r.pose[0:3] = list(tips[i, l] + np.array([0.02, -0.01, 0.0]))
            r.pose[3:7] = [1.0, 0.0, 0.0, 0.0]
            r.transform[:] = [0, 0, 0, 1, 0, 0, 0]
            r.swing_clearance = 0.02
    for e in (a, b):
        e.set_external_target(rows)
        e.step(2)
    ck, rec = a.checkpoint(), records(b)
    assert any(s.leg[l].step_plane_defined for s in rec[0] for l in range(L)), "no step plane is defined at capture time"
    for e in (a, b):
        e.set_velocity(-lin, ang * 0.5)
        e.set_tip_force(force * 0.0)
        e.step(40)
    a.restore(ck)
    host_restore(b, rec, None)
    same(a, b, "right after the restore")
    for e in (a, b):
        e.set_velocity(lin * 0.7, -ang)
        e.set_tip_force(force)
        e.step(30)
    same(a, b, "30 cycles after the restore")


def test_planner_mode_in_the_middle_of_a_plan_step(Engine):
    """Case 5d: planner mode under IMU posing, captured in the middle of a plan step - the LegPoser tips are state there (flag 8 of the auxiliary blob)."""
    from scipy.spatial.transform import Rotation as R
    p = default_hexapod_params("tripod")
    p.imu_posing, p.admittance_control = 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    n, L = 37, p.leg_count
    rng = np.random.default_rng(12)

    def imu_reading():
        e = np.stack([rng.uniform(-0.12, 0.12, n), rng.uniform(-0.12, 0.12, n), rng.uniform(-1, 1, n)], axis=1)
        q = R.from_euler("xyz", e).as_quat()
        return np.stack([q[:, 3], q[:, 0], q[:, 1], q[:, 2]], axis=1), rng.normal(0, 0.03, (n, 3))

    t = generate_tables(p)
    a, b = Engine(p, n, tables=t), Engine(p, n, tables=t)
    lin, ang, first = rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.5, 0.5, n), imu_reading()
    for e in (a, b):
        e.set_velocity(lin, ang)
        e.set_tip_force(np.full((n, L, 3), 1.5))
        e.set_imu(*first)
        e.step(80)
        e.set_planner_mode(True)
        for _ in range(600):
            pr, _ = e.execute_plan()
            if (pr == WAITING).all():
                break
        assert (pr == WAITING).all()
    cfg = a.joints()[0].reshape(n, L, -1) + rng.uniform(-0.1, 0.1, (n, L, 3))
    second, third, fourth = imu_reading(), imu_reading(), imu_reading()
    for e in (a, b):
        e.set_imu(*second)
        e.set_target_configuration(cfg)
        for _ in range(8):
            pr, _ = e.execute_plan()
        assert ((pr > 0) & (pr < 100)).any(), "no robot is in the middle of a plan step"
    ck, rec = a.checkpoint(), records(b)
    for e in (a, b):
        e.set_imu(*third)
        for _ in range(40):
            e.execute_plan()
    a.restore(ck)
    host_restore(b, rec, None)
    same(a, b, "right after the restore")
    out = []
    for e in (a, b):
        e.set_imu(*fourth)
        out.append([e.execute_plan() for _ in range(30)])
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(*out))
    same(a, b, "30 plan loops after the restore")


def test_update_behaves_as_a_fresh_checkpoint(Engine):
    """Case 6: checkpoint_update after more cycles; the device bytes held do not change (no records grew in between)."""
    (a, b), p, n = make(Engine, "6x3")
    ck = a.checkpoint()
    held = ck.nbytes
    first = inputs(p, n, 1)
    for e in (a, b):
        drive(e, first, 60)
    ck.update()
    rec = records(b)
    assert ck.nbytes == held
    other = inputs(p, n, 2)
    for e in (a, b):
        drive(e, other, 40)
    restore_and_compare(a, b, ck, rec, clone_map("shifted", n), p, n)


def test_refusals_change_nothing(Engine):
    """Case 7."""
    (a, b), p, n = make(Engine, "6x3")
    L = a.L
    restore = lambda e, ck, src=None, dev=0: L.shc_engine_restore_instances(e.h, ck.h, None if src is None else src.ctypes.data_as(C.c_void_p), dev)
    first = inputs(p, n, 1)
    for e in (a, b):
        drive(e, first, 60)
    ck, ckb = a.checkpoint(), b.checkpoint()
    drive(a, inputs(p, n, 2), 20)

    def refused(code, *args):
        before = state_bytes(a), a.get_aux_state()
        assert restore(*args) == code
        assert (state_bytes(a), a.get_aux_state()) == before

    refused(SHC_ERR_INVALID_ARG, a, ckb)                                  # another engine's checkpoint
    bad = np.arange(n, dtype=np.int64)
    bad[7] = n
    refused(SHC_ERR_INVALID_ARG, a, ck, bad)                              # a host map with an entry >= n
    with pytest.raises(ShcError):
        a.restore(ck, bad)
    with pytest.raises(ValueError):
        a.restore(ck, np.arange(n - 1))
    assert a.adjust_parameter(PARAM_SWING_HEIGHT, 0.03) == 0              # pending until its loop ...
    refused(SHC_ERR_UNSUPPORTED, a, ck)
    a.step(1)                                                             # ... and of another generation once served
    refused(SHC_ERR_UNSUPPORTED, a, ck)
    ck.update()
    assert restore(a, ck) == SHC_OK
    waiting = -1
    for _ in range(400):                                                  # a step-frequency change: asked every loop until it is accepted
        waiting = a.adjust_parameter(PARAM_STEP_FREQUENCY, 1.2)
        refused(SHC_ERR_UNSUPPORTED, a, ck)
        a.step(1)
        if waiting == 0:
            break
    assert waiting == 0
    refused(SHC_ERR_UNSUPPORTED, a, ck)
    ck.update()
    assert restore(a, ck) == SHC_OK
    a.set_velocity(np.zeros((n, 2)), np.zeros(n))                         # change_gait needs every robot stopped
    for _ in range(40):
        a.step(25)
        if a.change_gait(default_hexapod_params("tripod")) == 0:
            break
    else:
        pytest.fail("the robots did not stop")
    refused(SHC_ERR_UNSUPPORTED, a, ck)
    ck.update()
    assert restore(a, ck) == SHC_OK
    a.resident_begin(ring_depth=4, max_cycles=50)                        # resident mode owns the state
    try:
        assert restore(a, ck) == SHC_ERR_BUSY
        assert L.shc_engine_checkpoint_update(a.h, ck.h) == SHC_ERR_BUSY
    finally:
        a.resident_end()
    assert restore(a, ck) == SHC_OK
    b.close()                                                             # the engine is gone: its checkpoint answers with an error ...
    assert ckb.nbytes == 0
    assert L.shc_engine_restore_instances(a.h, ckb.h, None, 0) == SHC_ERR_INVALID_ARG
    assert L.shc_engine_checkpoint_update(a.h, ckb.h) == SHC_ERR_INVALID_ARG
    ckb.close()                                                           # ... and closing it afterwards is harmless
    with a.checkpoint() as scoped:
        assert scoped.nbytes > 0
    assert scoped.h is None
