"""GPU (-m gpu): the three-role form of the resident 6 x 3 loop (walker / model / helper wavefront per robot group, 384-thread workgroups:
shc_resident2_kernel<6, 3, F_C2 [| F_TIPF], true>) against set_* + shc_engine_step(1) on a twin engine, byte for byte - every cycle's q / qd from
the output ring, the complete state record and the odometry after resident_end - and the same loop with SHC_RESIDENT_TWO_ROLE=1 (the two-role
form of the same build).  Batch sizes: 1 robot (a single live group), 10 (one full wave), 11 (a partial second pair), 21 (a second workgroup
whose second pair is inactive).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params

pytestmark = pytest.mark.gpu

CYCLES = 64
HISTORY = 45          # ordinary launches before the loop starts: the robots are walking when it does
STOP = range(4, 30)   # a stretch of zero command
WS_STARTING, WS_MOVING, WS_STOPPING, WS_STOPPED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def Engine():
    from syropod_highlevel_controller_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    return engine.BatchEngine


def params():
    p = default_hexapod_params("tripod")
    p.step_frequency = 5.0   # a 24-iteration step cycle: STOPPING -> STOPPED -> STARTING -> MOVING fits the run
    return p


def state_bytes(eng):
    return bytes(memoryview(eng.get_state()).cast("B"))


def plan(n, efforts_live):
    """What every cycle of the run receives (the same for the twin engine and the loop)."""
    rng = np.random.default_rng(100 * n + int(efforts_live))
    base_l, base_a = rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n)
    cyc = []
    for c in range(CYCLES):
        k = 0.6 + 0.4 * np.sin(0.3 * c + np.arange(n))
        lin, ang = base_l * k[:, None] + 0.05 * rng.standard_normal((n, 2)), base_a * k + 0.05 * rng.standard_normal(n)   # a new command every cycle
        if c in STOP:
            lin, ang = np.zeros((n, 2)), np.zeros(n)
        d = {"velocity": (lin, ang), "pose_input": None, "pose_reset_mode": None, "joint_effort": None, "direct": False}
        if c in (33, 41):     # joystick body posing mid-run ...
            d["pose_input"] = (rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3)))
        if c == 47:           # ... a reset mode, and its release
            d["pose_reset_mode"] = rng.integers(1, 6, n).astype(np.int32)
        if c == 55:
            d["pose_reset_mode"] = np.zeros(n, dtype=np.int32)
        if efforts_live and c % 7 == 3:
            d["joint_effort"] = rng.normal(0, 0.5, (n, 18))
        cyc.append(d)
    cyc[37]["direct"] = True  # one launch-free post: velocity (+ joint efforts) straight from bound device arrays
    if efforts_live:
        cyc[37]["joint_effort"] = rng.normal(0, 0.5, (n, 18))
    return cyc, rng.normal(0, 0.5, (n, 18))


def prepare(Engine, n, efforts_live, e0, first):
    e = Engine(params(), n)
    e.set_pose_input(np.zeros((n, 3)), np.zeros((n, 3)))   # (the manual-pose group of the state is live from the first pose input on)
    if efforts_live:
        e.set_joint_effort(e0)
    e.set_velocity(*first)
    e.step(HISTORY)
    return e


_reference = {}


def reference(Engine, n, efforts_live):
    """The twin engine: set_* + shc_engine_step(1) per cycle; computed once per case, shared by the tests, never changed."""
    key = (n, efforts_live)
    if key not in _reference:
        cyc, e0 = plan(n, efforts_live)
        a = prepare(Engine, n, efforts_live, e0, cyc[0]["velocity"])
        joints, states, walk = [], [None], set()   # states[c]: (state record, odometry) after c cycles
        for c, d in enumerate(cyc):
            a.set_velocity(*d["velocity"])
            if d["pose_input"] is not None:
                a.set_pose_input(*d["pose_input"])
            if d["pose_reset_mode"] is not None:
                a.set_pose_reset_mode(d["pose_reset_mode"])
            if d["joint_effort"] is not None:
                a.set_joint_effort(d["joint_effort"])
            a.step(1)
            joints.append(a.joints())
            walk |= set(int(w) for w in a.body_state()[2])
            states.append((state_bytes(a), a.odometry().copy()))
        a.close()
        # the inputs do what they are there for: the general walk state machine with its stop predicates
        assert walk == {WS_STARTING, WS_MOVING, WS_STOPPING, WS_STOPPED}, walk
        _reference[key] = (cyc, e0, joints, states)
    return _reference[key]


def run_loop(Engine, n, efforts_live, stop_at, max_cycles):
    """The same cycles through one resident launch: ring posts released singly and in bursts (each waited for, so that the loop idles in
    between), one direct post; ended by resident_end right behind the release of the burst that reaches stop_at (the loop stops once it
    has run what was released), or by itself at max_cycles."""
    import torch
    cyc, e0, joints, states = reference(Engine, n, efforts_live)
    b = prepare(Engine, n, efforts_live, e0, cyc[0]["velocity"])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    lin_d, ang_d, eff_d = dev(cyc[37]["velocity"][0]), dev(cyc[37]["velocity"][1]), dev(cyc[37]["joint_effort"] if efforts_live else np.zeros((n, 18)))
    torch.cuda.current_stream().synchronize()
    b.resident_bind_inputs(0, velocity=(lin_d.data_ptr(), ang_d.data_ptr()), joint_effort=eff_d.data_ptr() if efforts_live else None)
    depth = 8
    b.resident_begin(ring_depth=depth, max_cycles=max_cycles)
    c, total = 0, min(CYCLES, max_cycles)
    bursts = [1, 1, 5, 1, 7, 2, 1, 6, 3, 1, 7, 1, 4]   # publish(k) bursts mixed with single ticks
    i = 0
    while c < total:
        k = min(bursts[i % len(bursts)], total - c)
        i += 1
        if any(d["direct"] for d in cyc[c:c + k]):
            k = 1 if cyc[c]["direct"] else [d["direct"] for d in cyc[c:c + k]].index(True)
        for d in cyc[c:c + k]:
            if d["direct"]:
                kw = {"velocity": True}
                if efforts_live:
                    kw["joint_effort"] = True
                assert b.resident_post(direct=0, **kw) == c   # (released at once)
            else:
                kw = {key: d[key] for key in ("velocity", "pose_input", "pose_reset_mode", "joint_effort") if d[key] is not None}
                b.resident_post(**kw)
        if not cyc[c]["direct"]:
            b.resident_publish(k)
        if c < stop_at <= c + k and stop_at < total:   # resident_end in mid-burst
            return b, b.resident_end(), joints, states
        b.resident_wait(c + k)
        for cc in range(c, c + k):
            q, qd = b.resident_joints(cc)
            assert np.array_equal(q, joints[cc][0]) and np.array_equal(qd, joints[cc][1]), f"cycle {cc}"
        c += k
    return b, b.resident_end(), joints, states


@pytest.mark.parametrize("form", ["helper", "two_role"])
@pytest.mark.parametrize("efforts_live", [False, True], ids=["c2", "c2_tipf"])
@pytest.mark.parametrize("n", [1, 10, 11, 21])
def test_three_role_loop_is_byte_identical_to_single_cycle_launches(Engine, monkeypatch, n, efforts_live, form):
    if form == "two_role":
        monkeypatch.setenv("SHC_RESIDENT_TWO_ROLE", "1")
    else:
        monkeypatch.delenv("SHC_RESIDENT_TWO_ROLE", raising=False)
    b, ran, joints, states = run_loop(Engine, n, efforts_live, stop_at=CYCLES, max_cycles=CYCLES + 10)
    assert ran == CYCLES
    assert state_bytes(b) == states[CYCLES][0]
    assert np.array_equal(b.odometry(), states[CYCLES][1]) and np.abs(states[CYCLES][1][:, :2]).max() > 1e-3
    b.close()


@pytest.mark.parametrize("how", ["max_cycles", "end_in_mid_burst"])
def test_three_role_loop_ends_at_its_bound_or_in_mid_burst(Engine, monkeypatch, how):
    """A run whose loop leaves by itself at max_cycles (= 40), and one that resident_end stops while a burst of several cycles is being run:
    the state after the cycles that ran is the twin's after as many."""
    monkeypatch.delenv("SHC_RESIDENT_TWO_ROLE", raising=False)
    n = 21
    if how == "max_cycles":
        b, ran, joints, states = run_loop(Engine, n, True, stop_at=CYCLES, max_cycles=40)
        assert ran == 40
    else:
        b, ran, joints, states = run_loop(Engine, n, True, stop_at=24, max_cycles=CYCLES + 10)
        assert ran == 24   # what was released, and nothing more
    q, qd = b.joints()
    assert np.array_equal(q, joints[ran - 1][0]) and np.array_equal(qd, joints[ran - 1][1])
    assert state_bytes(b) == states[ran][0] and np.array_equal(b.odometry(), states[ran][1])
    b.close()


_WHICH_FORM = """
import numpy as np
from syropod_highlevel_controller_amd import default_hexapod_params
from syropod_highlevel_controller_amd.engine import BatchEngine
e = BatchEngine(default_hexapod_params("tripod"), 11)
if {efforts}:
    e.set_joint_effort(np.full((11, 18), 0.1))
e.resident_begin(ring_depth=4, max_cycles=8)
e.resident_publish(3)
e.resident_wait(3)
assert e.resident_end() == 3
e.close()
"""


@pytest.mark.parametrize("form", ["helper", "two_role"])
@pytest.mark.parametrize("efforts_live", [False, True], ids=["c2", "c2_tipf"])
def test_which_kernel_form_a_process_launches(tmp_path, efforts_live, form):
    """Both forms are byte-identical by design, so the tests above cannot tell them apart: a fresh process logs the loop kernels it launches
    (SHC_KERNEL_LOG, "form legs joints features") - the 384-thread form by default, the two-role form under SHC_RESIDENT_TWO_ROLE=1."""
    log = tmp_path / "kernels.txt"
    env = dict(os.environ, SHC_KERNEL_LOG=str(log))
    env.pop("SHC_RESIDENT_TWO_ROLE", None)
    if form == "two_role":
        env["SHC_RESIDENT_TWO_ROLE"] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", _WHICH_FORM.format(efforts=efforts_live)], cwd=root, env=env, check=True, timeout=120)
    features = 1 | 64 | (32 if efforts_live else 0)   # F_MANUAL | F_ODOM [| F_TIPF]
    loops = [line.split() for line in log.read_text().splitlines() if line.startswith("resident")]
    assert loops == [["resident3" if form == "helper" else "resident2", "6", "3", str(features)]], loops
