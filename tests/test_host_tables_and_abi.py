"""CPU: the product's host init chain (libshc_batch.so, no GPU needed) against the oracle's, and the C ABI surface."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle_lib import OracleRobot
from syropod_highlevel_controller_amd import Params, Tables, default_hexapod_params, engine, synthetic_octopod_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def own_clock_auto_pose_params(gait, ready_at_phase_zero):
    """Auto posing with pose_frequency != -1.  The reference then poses the body while it is still starting up, and
    Leg::generateWorkspace runs at whatever pose the loop that reaches READY has (model.cpp:338): with the default 300
    start-up loops that pose is centimetres away from the one the start-up solve targeted, generateWorkspace finds the tip
    off its identity position (model.cpp:349-353) and returns a ZERO workspace - all velocity limits 0, the robot cannot
    walk (oracle and product agree on that).  ready_at_phase_zero picks time_to_start so that READY falls on pose phase 0."""
    p = default_hexapod_params(gait)
    p.auto_posing, p.pose_frequency = 1, 0.8
    for i in range(p.n_auto_posers):
        p.x_amplitudes[i], p.yaw_amplitudes[i] = 0.004 * (-1) ** i, 0.01
        if i % 2:
            p.gravity_amplitudes[i] = 0.008
    if ready_at_phase_zero:
        length = _pose_phase_length(p)
        loops = (299 // length) * length + 1              # <= 300; the last loop's master phase is (loops - 1) % length = 0
        p.time_to_start = loops * p.time_delta
    return p


def _pose_phase_length(p):
    base = p.pose_phase_length
    raw = (1.0 / p.pose_frequency) / p.time_delta
    k = int(raw / base)
    return (k if k % 2 == 0 else k + 1) * base   # roundToEvenInt (standard_includes.h:98)


def cases():
    for g in ("tripod", "wave", "ripple", "amble"):
        yield f"hexapod-{g}", default_hexapod_params(g)
    yield "octopod-ripple-5dof", synthetic_octopod_params("ripple", 5, 8)
    yield "quadruped-tripod-4dof", synthetic_octopod_params("tripod", 4, 4)
    p = default_hexapod_params("ripple")
    p.overlapping_walkspaces = 1  # walk_controller.cpp:101-104
    yield "hexapod-overlapping-walkspaces", p
    p = default_hexapod_params("tripod")
    p.step_frequency, p.body_clearance, p.time_delta = 0.6, 0.12, 0.01
    yield "hexapod-slow-steps-100Hz", p  # 600 start-up iterations: see START_UP_CHATTER below
    for g in ("tripod", "wave"):  # auto posing on its own clock already poses the body during the start-up loops
        for aligned in (False, True):
            p = own_clock_auto_pose_params(g, aligned)
            yield f"hexapod-{g}-auto-pose-own-clock" + ("-ready-at-phase-0" if aligned else ""), p
    for g, legs, dof in (("tripod", 6, 3), ("ripple", 6, 4)):  # rough terrain mode: the layered workspace (model.cpp:309-510)
        p = default_hexapod_params(g) if dof == 3 else synthetic_octopod_params(g, dof, legs)
        p.rough_terrain_mode = 1
        yield f"rough-terrain-{legs}x{dof}-{g}", p
    for name, (dof, legs, gait) in (("octopod-5dof-gravity-aligned-tips", (5, 8, "ripple")), ("hexapod-4dof-gravity-aligned-tips", (4, 6, "tripod"))):
        p = synthetic_octopod_params(gait, dof, legs)
        p.gravity_aligned_tips = 1  # rotation-constrained start-up solve (model.cpp:880-900)
        yield name, p


@pytest.mark.parametrize("name,p", list(cases()), ids=[c[0] for c in cases()])
def test_tables_match_oracle(name, p):
    o = OracleRobot(p).tables()
    t = engine.generate_tables(p)
    L, NJ = p.leg_count, p.leg_dof[0]
    for f in ("period", "swing_period", "stance_period", "stance_end", "swing_start", "swing_end", "stance_start"):
        assert getattr(o.step, f) == getattr(t.step, f)                      # integers: bit-exact
    assert o.step.frequency == t.step.frequency
    assert list(o.phase_offset)[:L] == list(t.phase_offset)[:L]
    assert (o.pose_phase_length, o.pose_normaliser, o.auto_pose_reference_leg) == (t.pose_phase_length, t.pose_normaliser, t.auto_pose_reference_leg)
    dq = max(abs(o.default_joint_position[l][j] - t.default_joint_position[l][j]) for l in range(L) for j in range(NJ))
    # Start-up solve: a fixed number of DLS steps (time_to_start / time_delta) of an iteration that amplifies rounding
    # differences by ~1.1x per step (tests/test_oracle_conditioning.py).  The yardstick is the oracle itself: the product's
    # configuration must be as close to the oracle's as the oracle's own fast-math build is (x20, floor 1e-9 rad) - 1e-15 at
    # 100 steps, 1e-9 at the default 300, the chatter amplitude (mrad) beyond ~350 steps where the iteration is
    # ill-conditioned.  Everything derived from the configuration (workspace, walkspace, limits) is compared tightly below.
    from test_oracle_conditioning import dq as dq_of, twin_tables
    steps = max(1, round(p.time_to_start / p.time_delta))
    START_UP_CHATTER = max(20 * dq_of(o, twin_tables(p), L, NJ), 1e-9)
    if steps > 300:
        START_UP_CHATTER = max(START_UP_CHATTER, 5e-3)
    print(f"{name}: {steps} start-up steps, |product - oracle| = {dq:.2e} rad (bound {START_UP_CHATTER:.2e})")
    assert dq < START_UP_CHATTER
    for l in range(L):
        np.testing.assert_allclose(list(t.workspace_radius[l]), list(o.workspace_radius[l]), atol=1e-9)
    for f in ("walkspace", "max_linear_speed", "max_angular_speed", "max_linear_acceleration", "max_angular_acceleration"):
        np.testing.assert_allclose(list(getattr(t, f)), list(getattr(o, f)), rtol=1e-9, atol=1e-12)
        if "own-clock" in name and "phase-0" not in name:
            assert all(v == 0 or v > 1e9 for v in getattr(t, f))  # zero workspace: speeds 0, accelerations UNASSIGNED
        else:
            assert all(v > 0 for v in getattr(t, f))


def test_library_exports_every_declared_symbol():
    declared = set(engine.HEADER.functions)   # (tests/test_abi_header.py holds the reader to a crude count of the header's own text)
    assert declared == set(engine.EXPORTED_SYMBOLS), declared ^ set(engine.EXPORTED_SYMBOLS)
    lib = C.CDLL(engine.build_library())
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert lib.shc_abi_version() == 6


def test_struct_layouts_match_the_library():
    lib = engine.lib()
    assert lib.shc_sizeof_params() == C.sizeof(Params)
    assert lib.shc_sizeof_tables() == C.sizeof(Tables)


def test_unsupported_parameters_are_rejected():
    p = default_hexapod_params("tripod")
    p.leg_dof[2] = 6                     # joints per leg: 3..5
    with pytest.raises(engine.ShcError):
        engine.generate_tables(p)
    from syropod_highlevel_controller_amd import synthetic_mixed_dof_params
    p = synthetic_mixed_dof_params("ripple")
    p.gravity_aligned_tips = 1           # the reference decides per leg there (> 3 joints: tip rotation; leg 0 <= 3 joints: tip-align pose): supported
    engine.generate_tables(p)


def test_mixed_dof_host_tables_match_the_oracle():
    """A robot whose legs differ in DOF (3 / 5 / 4 / 3 / 5 / 4): the product's host init chain pads the shorter legs behind their tips,
    the oracle runs every leg with its own joint count - start-up configuration, workspaces and limit tables agree (100 start-up steps)."""
    from syropod_highlevel_controller_amd import synthetic_mixed_dof_params
    p = synthetic_mixed_dof_params("ripple")
    p.time_to_start = 2.0
    t, o = engine.generate_tables(p), OracleRobot(p).tables()
    for l in range(p.leg_count):
        d = p.leg_dof[l]
        dq = np.abs(np.array(t.default_joint_position[l][:d]) - np.array(o.default_joint_position[l][:d])).max()
        assert dq < (1e-8 if d == 5 else 1e-12), (l, d, dq)
        assert all(v == 0.0 for v in t.default_joint_position[l][d:5])
        np.testing.assert_allclose(list(t.workspace_radius[l]), list(o.workspace_radius[l]), atol=1e-9)
    for f in ("walkspace", "max_linear_speed", "max_angular_speed", "max_linear_acceleration", "max_angular_acceleration"):
        np.testing.assert_allclose(list(getattr(t, f)), list(getattr(o, f)), rtol=1e-9, atol=1e-12)


def test_no_cpu_fallback_without_a_device():
    """The product path must fail loudly when there is no HIP device (no silent CPU path)."""
    if engine.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(engine.ShcError):
        engine.BatchEngine(default_hexapod_params("tripod"), 8)
    h = C.c_void_p()
    p = default_hexapod_params("tripod")
    rc = engine.lib().shc_engine_create(C.byref(p), 8, 0, None, C.byref(h))
    assert rc == engine.SHC_ERR_NO_DEVICE and not h.value


def test_product_does_not_reference_the_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "syropod_highlevel_controller_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(root, f)).read()
                assert "liboracle" not in src and "oracle_lib" not in src and "shc_oracle" not in src, f


_NULL_SWEEP = r'''
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from syropod_highlevel_controller_amd import engine
lib = C.CDLL(engine.build_library())
decls, pointers = json.loads(sys.argv[2]), sys.argv[3] == "buffers"
scratch = C.create_string_buffer(1 << 20)          # what a pointer argument points at in the second pass (zeroed, larger than any one call reads)
INT = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double}
out = {}
for name, ret, args in decls:
    f = getattr(lib, name)
    f.restype = INT[ret]
    types, vals = [C.c_void_p], [None]
    for a in args[1:]:
        if "*" in a:
            types.append(C.c_void_p)
            vals.append(C.addressof(scratch) if pointers else None)
        else:
            t = INT[a]
            types.append(t)
            vals.append(t(1 if pointers else 0))
    f.argtypes = types
    print("calling", name, flush=True)              # (a crash names its entry point in the child's output)
    out[name] = int(f(*vals))
print("RESULT " + json.dumps(out), flush=True)
'''


def _engine_entry_points():
    """Every shc_engine_* declaration of the public header that takes the engine first: (name, return type, [argument types])."""
    return [(name, ret, [t for t, _ in params]) for name, (ret, params) in engine.HEADER.functions.items()
            if name.startswith("shc_engine_") and ret in ("int", "int64_t") and params and params[0] in (("shc_engine *", "e"), ("const shc_engine *", "e"))]


@pytest.mark.parametrize("pointers", ["null", "buffers"])
def test_every_entry_point_rejects_a_null_engine(pointers):
    """A NULL engine with NULL / zero arguments (and again with valid host buffers and ones): every shc_engine_* call that takes the engine first
    returns SHC_ERR_INVALID_ARG before it touches anything - no call dereferences first (the state transfer flushed a pending step-frequency remap
    through the engine pointer before its check).  The exceptions: shc_engine_destroy(NULL) is a no-op, and the size / index queries that return
    int64_t answer "nothing" (0 instances, 0 bytes, index -1).  The calls run in a fresh interpreter so that a crash fails this test instead of the suite."""
    import json
    import subprocess
    import sys
    decls = _engine_entry_points()
    assert len(decls) >= 60 and {"shc_engine_get_state", "shc_engine_set_state", "shc_engine_adjust_parameter"} <= {d[0] for d in decls}
    r = subprocess.run([sys.executable, "-c", _NULL_SWEEP, ROOT, json.dumps(decls), pointers], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0, f"the child died (status {r.returncode}) after: {lines[-1:] }\n{r.stderr[-2000:]}"
    got = json.loads(next(l for l in lines if l.startswith("RESULT "))[7:])
    expect = {name: engine.SHC_ERR_INVALID_ARG for name, _, _ in decls}
    expect["shc_engine_destroy"] = engine.SHC_OK
    expect.update(shc_engine_instances=0, shc_engine_aux_state_bytes=0, shc_engine_joint_index=-1)   # (the three size / index queries: nothing there)
    wrong = {k: (v, expect[k]) for k, v in got.items() if v != expect[k]}
    assert not wrong, wrong
