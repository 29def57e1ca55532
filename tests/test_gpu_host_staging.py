"""GPU: the host-array forms of the entry points after the move onto one staging scope (csrc/shc_stage.hpp: StageArena + HostCall).

6x3 hexapods at n = 1 and n = 23 (three wavefronts of ten robots, the last one partial).  The engine's staging arena holds
n * 6 * 3 * 8 + n * 64 + SHC_MAX_LEGS * SHC_MAX_JOINTS * 8 + 4096 bytes: 4 688 at n = 1 and 9 264 at n = 23 (`arena_bytes`, asserted below against the
record sizes).  At n = 1 the leg-state messages (6 * 512 = 3 072 B) and the frame transforms (6 * 336 + 160 = 2 176 B) fit the arena; at n = 23 they
need 70 656 B and 50 048 B and take the temporary path.  get_state needs 4 744 B per robot: 56 B more than the arena of ONE robot holds, so it takes
the temporary path at both sizes (109 112 B at n = 23).  Every other array of these tests fits the arena at both sizes.

(a) one entry point of each family in its host form on one engine and in its device form (torch tensors) on a twin - where there is no device
    form, the host form on both: outputs byte-equal, and get_state + get_aux_state byte-equal three cycles later.
(b) the entry points that call other entry points while their own staged data is live: set_joint_states_msg(position, effort) against the two
    simpler calls on a twin; toggle_leg_state on a batch where some robots need the ordinary cycle, and the direct start-up through its last call
    (which runs the first control cycle), against tests/golden/host_staging_golden.npz - what the commit before the staging scope returned for the
    same calls on an MI355X (`python tests/test_gpu_host_staging.py OUT.npz` records it)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "host_staging_golden.npz")
pytestmark = pytest.mark.gpu


def arena_bytes(n, legs=6, dof=3):
    from syropod_highlevel_controller_amd.params import SHC_MAX_JOINTS, SHC_MAX_LEGS
    return n * legs * max(dof, 3) * 8 + n * 8 * 8 + SHC_MAX_LEGS * SHC_MAX_JOINTS * 8 + 4096


def hexapod():
    from syropod_highlevel_controller_amd import default_hexapod_params
    p = default_hexapod_params("tripod")
    p.rough_terrain_mode = 1   # walking robots take external targets
    return p


def state_bytes(e):
    return bytes(e.get_state())


def test_which_forms_leave_the_arena():
    from syropod_highlevel_controller_amd.engine import BODY_FRAMES_DTYPE, LEG_FRAMES_DTYPE, LEG_STATE_MSG_DTYPE, InstanceState
    msgs, frames, state = 6 * LEG_STATE_MSG_DTYPE.itemsize, 6 * LEG_FRAMES_DTYPE.itemsize + BODY_FRAMES_DTYPE.itemsize, C.sizeof(InstanceState)
    assert (arena_bytes(1), arena_bytes(23)) == (4688, 9264)
    assert msgs <= arena_bytes(1) and frames <= arena_bytes(1) and state > arena_bytes(1)
    assert 23 * msgs > arena_bytes(23) and 23 * frames > arena_bytes(23) and 23 * state > arena_bytes(23)


@pytest.mark.parametrize("n", [1, 23])
def test_host_forms_against_device_forms(n):
    import torch
    from syropod_highlevel_controller_amd.engine import (BODY_FRAMES_DTYPE, HEALTH_ALL, LEG_FRAMES_DTYPE, LEG_STATE_MSG_DTYPE, ROBOT_HEALTH_DTYPE, BatchEngine,
                                                         HealthCriteria, _check)
    from syropod_highlevel_controller_amd.params import ExternalTarget
    p = hexapod()
    L, D = 6, 3
    rng = np.random.default_rng(n)
    a, b = BatchEngine(p, n), BatchEngine(p, n)   # a: host forms, b: device forms
    lib = a.L
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    host = lambda t: t.cpu().numpy()
    try:
        # ---- a robot setter, a leg setter, the joint-state message with position and effort
        lin, ang = rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.4, 0.4, n)
        force = np.abs(rng.normal(0, 2.0, (n, L, 3)))
        raw, eff = rng.normal(0, 0.3, (n, L * D)), rng.normal(0, 0.5, (n, L * D))
        a.set_velocity(lin, ang)
        a.set_tip_force(force)
        a.set_joint_states_msg(raw, None, eff)
        d_in = [dev(x) for x in (lin, ang, force, raw, eff)]
        _check(lib.shc_engine_set_velocity(b.h, ptr(d_in[0]), ptr(d_in[1]), 1), "set_velocity")
        _check(lib.shc_engine_set_tip_force(b.h, ptr(d_in[2]), 1), "set_tip_force")
        _check(lib.shc_engine_set_joint_states_msg(b.h, ptr(d_in[3]), None, ptr(d_in[4]), 1), "set_joint_states_msg")
        for e in (a, b):
            e.step(7)
        assert state_bytes(a) == state_bytes(b), "setters: host and device forms leave different states"

        # ---- per-leg calls with an input and an output, on a range that is not the whole batch at n = 23
        first, count = (0, 1) if n == 1 else (3, 19)
        rows = count * L
        delta = rng.normal(0, 0.004, (rows, 6))
        jd_a = a.leg_solve_ik(delta, first=first, count=count)
        d_delta, d_jd = dev(delta), torch.zeros(rows, D, dtype=torch.float64, device="cuda")
        _check(lib.shc_leg_solve_ik(b.h, first, count, -1, ptr(d_delta), 0, ptr(d_jd), 1), "leg_solve_ik")
        assert jd_a.tobytes() == host(d_jd).tobytes(), "leg_solve_ik"
        prox_a = a.leg_update_joint_positions(jd_a, first=first, count=count)
        d_prox = torch.zeros(rows, dtype=torch.float64, device="cuda")
        _check(lib.shc_leg_update_joint_positions(b.h, first, count, -1, ptr(d_jd), 0, ptr(d_prox), 1), "leg_update_joint_positions")
        assert prox_a.tobytes() == host(d_prox).tobytes(), "leg_update_joint_positions"
        fk_a = a.leg_apply_fk(None, first=first, count=count)
        d_fk = torch.zeros(rows, 7, dtype=torch.float64, device="cuda")
        _check(lib.shc_leg_apply_fk(b.h, first, count, -1, None, ptr(d_fk), 1), "leg_apply_fk")
        assert fk_a.tobytes() == host(d_fk).tobytes(), "leg_apply_fk"

        # ---- leg_step_to_position: target_pose has one row per INSTANCE, the other arrays one per (instance, leg); int32 progress rows
        target = fk_a + np.concatenate([rng.normal(0, 0.01, (rows, 3)), np.zeros((rows, 4))], axis=1)
        pose = np.tile([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], (count, 1)) + np.concatenate([rng.normal(0, 0.005, (count, 3)), np.zeros((count, 4))], axis=1)
        for it in range(3):
            tip_a, prog_a = a.leg_step_to_position(target, pose, 0.02, 0.2, first=first, count=count)
            d_t, d_p = dev(target), dev(pose)
            d_tip, d_prog = torch.zeros(rows, 7, dtype=torch.float64, device="cuda"), torch.full((rows,), -7, dtype=torch.int32, device="cuda")
            _check(lib.shc_leg_step_to_position(b.h, first, count, -1, ptr(d_t), ptr(d_p), 0.02, 0.2, 1, ptr(d_tip), ptr(d_prog), 1), "leg_step_to_position")
            assert tip_a.tobytes() == host(d_tip).tobytes() and prog_a.tobytes() == host(d_prog).tobytes(), ("leg_step_to_position", it)
        assert state_bytes(a) == state_bytes(b), "per-leg calls: host and device forms leave different states"

        # ---- no device form: the host form on both.  Manual inputs (six arrays in one scope), external targets set and read back
        prim, sec = rng.integers(0, L, n).astype(np.int32), rng.integers(0, L, n).astype(np.int32)
        vel, pos = rng.uniform(-1, 1, (2, n, 3)), rng.uniform(-0.05, 0.05, (2, n, 3))
        ext = (ExternalTarget * (n * L))()
        for i, r in enumerate(ext):
            r.pose[:] = list(rng.normal(0, 0.1, 3)) + [1.0, 0.0, 0.0, 0.0]
            r.transform[:] = list(rng.normal(0, 0.1, 3)) + [1.0, 0.0, 0.0, 0.0]
            r.swing_clearance, r.defined, r.frame_is_odom_ideal = 0.03 + 0.001 * i, int(i % 5 != 0), int(i % 2)
        got = []
        for e in (a, b):
            e.set_manual_inputs(prim, vel[0], pos[0], sec, vel[1], pos[1])
            ignored = e.set_external_target(ext)
            got.append((ignored, bytes(e.get_external_target()), bytes(e.get_external_target(which=2)), e.leg_manipulation_state().tobytes()))
        assert got[0] == got[1], "set_manual_inputs / set_external_target / get_external_target differ between two engines"
        assert got[0][1] != bytes((ExternalTarget * (n * L))()), "no external target was taken: the read-back compares nothing"
        for e in (a, b):
            e.step(2)

        # ---- scan_health, leg_state_msgs, frame_transforms, joint_commands: host arrays against device buffers
        select, near = HEALTH_ALL, 0.9   # (a wide near-limit band: some robots are selected, the list has a length to come back first)
        health_a, sel_a = a.scan_health(select, near)
        d_health = torch.zeros(n * ROBOT_HEALTH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_map, d_sel, d_nsel = (torch.full((k,), -5, dtype=torch.int64, device="cuda") for k in (n, n, 1))
        b.scan_health(select, near, out_health=d_health, out_restore_map=d_map, out_selected=d_sel, out_n_selected=d_nsel)
        n_sel = int(d_nsel.cpu()[0])
        assert health_a.tobytes() == host(d_health).tobytes() and n_sel == len(sel_a) and np.array_equal(sel_a, host(d_sel)[:n_sel]), "scan_health"
        map_a = np.zeros(n, dtype=np.int64)
        crit = HealthCriteria(select, 0, near, 0.0)
        _check(lib.shc_engine_scan_health(a.h, 0, n, C.byref(crit), None, map_a.ctypes.data_as(C.c_void_p), None, None, 0), "scan_health")
        assert np.array_equal(map_a, host(d_map)), "scan_health: restore map"

        msgs_a = a.leg_state_msgs()
        d_msgs = torch.zeros(n * L * LEG_STATE_MSG_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        b.leg_state_msgs(out=d_msgs.data_ptr())
        assert msgs_a.tobytes() == host(d_msgs).tobytes(), "leg_state_msgs"

        for frame in ("base_link", "odom_ideal"):
            lf_a, bf_a = a.frame_transforms(frame=frame)
            d_lf = torch.zeros(n * L * LEG_FRAMES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_bf = torch.zeros(n * BODY_FRAMES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            b.frame_transforms(frame=frame, out_legs=d_lf.data_ptr(), out_body=d_bf.data_ptr())
            assert lf_a.tobytes() == host(d_lf).tobytes() and bf_a.tobytes() == host(d_bf).tobytes(), ("frame_transforms", frame)

        cmd_a = a.joint_commands()
        d_cmd = [torch.zeros(n, L * D, dtype=torch.float64, device="cuda") for _ in range(4)]
        _check(lib.shc_engine_get_joint_commands(b.h, *[ptr(t) for t in d_cmd], 1), "get_joint_commands")
        for k in range(4):
            assert cmd_a[k].tobytes() == host(d_cmd[k]).tobytes(), ("joint_commands", k)
        assert any(np.any(c != 0) for c in cmd_a)

        # ---- and the engines go on as one
        for e in (a, b):
            e.step(3)
        assert state_bytes(a) == state_bytes(b), "get_state differs three cycles later"
        assert bytes(a.get_aux_state()) == bytes(b.get_aux_state()), "get_aux_state differs three cycles later"
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("n", [1, 23])
def test_joint_states_msg_with_effort_is_its_two_simpler_calls(n):
    """set_joint_states_msg(position, effort) stages the joint offsets and the positions, then calls set_joint_effort, which stages again."""
    from syropod_highlevel_controller_amd.engine import BatchEngine
    p = hexapod()
    rng = np.random.default_rng(100 + n)
    a, b = BatchEngine(p, n), BatchEngine(p, n)
    try:
        lin, ang = rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.4, 0.4, n)
        for k in range(3):
            raw, eff = rng.normal(0, 0.3, (n, 18)), rng.normal(0, 0.5, (n, 18))
            a.set_joint_states_msg(raw, None, eff)
            b.set_joint_states_msg(raw, None, None)
            b.set_joint_effort(eff)
            for e in (a, b):
                e.set_velocity(lin, ang)
                e.step(3)
            assert a.leg_state_msgs().tobytes() == b.leg_state_msgs().tobytes(), k   # (the measured positions show in actual_tip_pose, the efforts in joint_efforts)
            assert state_bytes(a) == state_bytes(b), k
    finally:
        a.close()
        b.close()


# ---- the nesting callers without a simpler equivalent: what the commit before the staging scope returned

def nesting_record():
    """toggle_leg_state over 40 loops on 23 robots - 12 walk (told to stop first: their loop is the ordinary cycle, run from inside the call), 11 stand,
    every third robot makes no request - and a direct start-up through its last call."""
    from syropod_highlevel_controller_amd.engine import BatchEngine
    n, L = 23, 6
    out = {}
    e = BatchEngine(hexapod(), n)
    try:
        rng = np.random.default_rng(5)
        lin, ang = rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.5, 0.5, n)
        lin[12:], ang[12:] = 0.0, 0.0
        e.set_velocity(lin, ang)
        e.step(40)
        sel = np.array([i % L if i % 3 else -1 for i in range(n)], dtype=np.int32)
        pending, results = sel >= 0, []
        for _ in range(40):
            res = e.toggle_leg_state(np.where(pending, sel, -1).astype(np.int32))
            results.append(res.copy())
            still = res == -1
            if still.any():   # (the node zeroes the velocity inputs of a robot that is told to stop)
                lin[still], ang[still] = 0.0, 0.0
                e.set_velocity(lin, ang)
            pending &= ~((res == 1) | (res == 2))
        out["toggle_results"] = np.stack(results)
        out["toggle_manipulation_state"] = e.leg_manipulation_state()
        out["toggle_joints"] = np.stack(e.joints())
        out["toggle_state"] = np.frombuffer(state_bytes(e), dtype=np.uint8)
        out["toggle_aux"] = np.frombuffer(bytes(e.get_aux_state()), dtype=np.uint8)
    finally:
        e.close()
    e = BatchEngine(hexapod(), n)
    try:
        e.begin_direct_startup()
        progress = []
        while not progress or progress[-1] != 100:
            assert len(progress) < 5000
            progress.append(e.direct_startup())
        out["startup_progress"] = np.array(progress, dtype=np.int32)
        out["startup_joints"] = np.stack(e.joints())
        out["startup_state"] = np.frombuffer(state_bytes(e), dtype=np.uint8)
    finally:
        e.close()
    return out


def test_nesting_callers_against_the_recorded_parent():
    want, got = np.load(GOLDEN), nesting_record()
    assert sorted(want.files) == sorted(got)
    res = want["toggle_results"]
    assert (res[0][:12] == -1).sum() > 0 and (res[0][12:] != -1).all(), "the recorded batch mixes robots that need the ordinary cycle with robots that do not"
    for k in want.files:
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape and want[k].tobytes() == got[k].tobytes(), k


if __name__ == "__main__":   # record the golden: with the package of the commit whose behaviour is the reference on PYTHONPATH
    np.savez_compressed(sys.argv[1], **nesting_record())
