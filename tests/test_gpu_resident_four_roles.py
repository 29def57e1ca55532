"""GPU (-m gpu): the four-role form of the resident 6 x 3 loop (walker / model / front helper / pose helper wavefront per robot group, 512-thread
workgroups: shc_resident2_kernel<6, 3, F_C2 [| F_TIPF], 2>) against set_* + shc_engine_step(1) on a twin engine, byte for byte: every cycle's q / qd
from the output ring, the complete state record and the odometry after resident_end.

The front helper runs nothing but the velocity front, the pose helper the pose, the odometry and the leader's duty; they meet the walker through the
front / pose flags and the per-iteration barrier only.  What the runs reach:
  - inputs: a stretch of ring posts (a new command every cycle, joystick posing, a reset mode and its release, joint efforts), a stretch of bare publishes
    (held inputs), a stretch of direct posts from two bound sets whose arrays change before every post;
  - releases: one tick at a time, each waited for (every real iteration has bubbles around it), and bursts of several cycles;
  - ends: resident_end behind everything, resident_end in the middle of a released burst, the loop's own max_cycles;
  - walking: the even robots are stopped and start again inside the window, the odd ones stop later and stay stopped through the held stretch - the
    non-steady path of the walker's wait for the front, and wavefronts whose robots are in different walk states.
Batch sizes: 1 robot (the second pair of the workgroup is inactive: its helper wavefronts only keep the barriers), 9 and 10 (a partial and an exactly
full wave), 11 (a second pair with a single robot), 21 (a second workgroup whose last pair is partial).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params

pytestmark = pytest.mark.gpu

CYCLES = 56
HISTORY = 45                # ordinary launches before the loop starts: the robots are walking when it does
STOP_EVEN = range(2, 24)    # zero command for the even robots: they stop, and start again at cycle 24
STOP_ODD = range(14, 36)    # ... and for the odd ones: they stop later and stay stopped until the direct posts begin
HELD = range(30, 36)        # bare publishes: every input held
DIRECT = range(38, 50)      # direct posts, bound sets 0 and 1 in turn, their arrays rewritten before every post
WS_STARTING, WS_MOVING, WS_STOPPING, WS_STOPPED = 0, 1, 2, 3
SIZES = [1, 9, 10, 11, 21]


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
    """What every cycle of the run receives (the same for the twin engine and the loop).  how: "post" (ring post), "held" (bare publish), "direct"."""
    rng = np.random.default_rng(4000 + 100 * n + int(efforts_live))
    base_l, base_a = rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n)
    even = np.arange(n) % 2 == 0
    cyc = []
    for c in range(CYCLES):
        k = 0.6 + 0.4 * np.sin(0.3 * c + np.arange(n))
        lin, ang = base_l * k[:, None] + 0.05 * rng.standard_normal((n, 2)), base_a * k + 0.05 * rng.standard_normal(n)   # a new command every cycle
        zero = (even & (c in STOP_EVEN)) | (~even & (c in STOP_ODD))
        lin[zero], ang[zero] = 0.0, 0.0
        how = "held" if c in HELD else "direct" if c in DIRECT else "post"
        d = {"how": how, "velocity": (lin, ang), "pose_input": None, "pose_reset_mode": None, "joint_effort": None}
        if c in (8, 27):      # joystick body posing mid-run ...
            d["pose_input"] = (rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3)))
        if c == 18:           # ... a reset mode, and its release
            d["pose_reset_mode"] = rng.integers(1, 6, n).astype(np.int32)
        if c == 52:
            d["pose_reset_mode"] = np.zeros(n, dtype=np.int32)
        if efforts_live and how != "held" and (how == "direct" or c % 5 == 3):
            d["joint_effort"] = rng.normal(0, 0.5, (n, 18))
        cyc.append(d)
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
        joints, states, walk = [], [None], []   # states[c]: (state record, odometry) after c cycles; walk[c]: every robot's walk state after cycle c
        for d in cyc:
            if d["how"] != "held":
                a.set_velocity(*d["velocity"])
                if d["pose_input"] is not None:
                    a.set_pose_input(*d["pose_input"])
                if d["pose_reset_mode"] is not None:
                    a.set_pose_reset_mode(d["pose_reset_mode"])
                if d["joint_effort"] is not None:
                    a.set_joint_effort(d["joint_effort"])
            a.step(1)
            joints.append(a.joints())
            walk.append(np.array(a.body_state()[2], dtype=np.int64).copy())
            states.append((state_bytes(a), a.odometry().copy()))
        a.close()
        # the inputs do what they are there for: a robot that stops walking inside the window and one that starts (one robot: it does both) ...
        walk = np.stack(walk)
        stops = ((walk[:-1] == WS_MOVING) & (walk[1:] == WS_STOPPING)).any(axis=0)
        starts = ((walk[:-1] == WS_STOPPED) & (walk[1:] == WS_STARTING)).any(axis=0)
        assert stops.any() and starts.any(), (stops, starts)
        assert set(walk.ravel().tolist()) == {WS_STARTING, WS_MOVING, WS_STOPPING, WS_STOPPED}
        if n > 1:             # ... and cycles in which robots of one wavefront are in different walk states
            assert (walk[:, 0] != walk[:, 1]).any()
        _reference[key] = (cyc, e0, joints, states)
    return _reference[key]


def releases_of(cyc, total, sizes):
    """(first cycle, length) of every release.  Posts fill the next unposted cycle, so a burst is posted cycles followed by bare ones; a direct post is a
    release of its own."""
    out, c, i = [], 0, 0
    while c < total:
        k, j = min(sizes[i % len(sizes)], total - c), 1
        i += 1
        while j < k and cyc[c]["how"] != "direct" and cyc[c + j]["how"] != "direct" and not (cyc[c + j]["how"] == "post" and cyc[c + j - 1]["how"] == "held"):
            j += 1
        out.append((c, j))
        c += j
    return out


TICKS, BURSTS = [1], [1, 1, 5, 1, 7, 2, 1, 6, 3, 1, 7, 1, 4]


def run_loop(Engine, n, efforts_live, sizes, stop_at, max_cycles):
    """The same cycles through one resident launch, each release waited for (so that the loop idles in between) and every cycle's q / qd compared as it
    completes; ended by resident_end right behind the release of the burst that reaches stop_at (the loop stops once it has run what was released), or by
    itself at max_cycles.  Returns (engine, cycles run, cycles released, the twin's joints, the twin's states)."""
    import torch
    cyc, e0, joints, states = reference(Engine, n, efforts_live)
    b = prepare(Engine, n, efforts_live, e0, cyc[0]["velocity"])
    sets = [(torch.zeros((n, 2), dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"),
             torch.zeros((n, 18), dtype=torch.float64, device="cuda")) for _ in range(2)]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.current_stream().synchronize()
    for i, (lin_d, ang_d, eff_d) in enumerate(sets):
        b.resident_bind_inputs(i, velocity=(lin_d.data_ptr(), ang_d.data_ptr()), joint_effort=eff_d.data_ptr() if efforts_live else None)
    b.resident_begin(ring_depth=8, max_cycles=max_cycles)
    total = min(CYCLES, max_cycles)
    for c, k in releases_of(cyc, total, sizes):
        for cc, d in enumerate(cyc[c:c + k], start=c):
            if d["how"] == "direct":   # (every earlier cycle has completed, and the joint efforts in force are the other set's: nothing reads what is rewritten here)
                lin_d, ang_d, eff_d = sets[cc & 1]
                lin_d.copy_(dev(d["velocity"][0]))
                ang_d.copy_(dev(d["velocity"][1]))
                if efforts_live:
                    eff_d.copy_(dev(d["joint_effort"]))
                torch.cuda.current_stream().synchronize()   # (a STREAM synchronisation: a device-wide one would wait for the resident loop itself)
                kw = {"velocity": True}
                if efforts_live:
                    kw["joint_effort"] = True
                assert b.resident_post(direct=cc & 1, **kw) == cc   # (released at once)
            elif d["how"] == "post":
                b.resident_post(**{key: d[key] for key in ("velocity", "pose_input", "pose_reset_mode", "joint_effort") if d[key] is not None})
        if cyc[c]["how"] != "direct":
            b.resident_publish(k)
        if c < stop_at <= c + k and stop_at < total:   # resident_end in mid-burst
            return b, b.resident_end(), c + k, joints, states
        b.resident_wait(c + k)
        for cc in range(c, c + k):
            q, qd = b.resident_joints(cc)
            assert np.array_equal(q, joints[cc][0]) and np.array_equal(qd, joints[cc][1]), f"cycle {cc}"
    return b, b.resident_end(), total, joints, states


def check_end(b, ran, joints, states):
    q, qd = b.joints()
    assert np.array_equal(q, joints[ran - 1][0]) and np.array_equal(qd, joints[ran - 1][1])
    assert state_bytes(b) == states[ran][0]
    assert np.array_equal(b.odometry(), states[ran][1]) and np.abs(states[ran][1][:, :2]).max() > 1e-3
    b.close()


@pytest.fixture(autouse=True)
def default_form(monkeypatch):
    monkeypatch.delenv("SHC_RESIDENT_TWO_ROLE", raising=False)
    monkeypatch.delenv("SHC_RESIDENT_THREE_ROLE", raising=False)


@pytest.mark.parametrize("release", ["ticks", "bursts"])
@pytest.mark.parametrize("efforts_live", [False, True], ids=["c2", "c2_tipf"])
@pytest.mark.parametrize("n", SIZES)
def test_four_role_loop_is_byte_identical_to_single_cycle_launches(Engine, n, efforts_live, release):
    """ticks: every cycle is released alone and waited for - bubbles between all real iterations; bursts: publish(k) releases mixed with single ticks."""
    b, ran, released, joints, states = run_loop(Engine, n, efforts_live, TICKS if release == "ticks" else BURSTS, stop_at=CYCLES, max_cycles=CYCLES + 10)
    assert ran == released == CYCLES
    check_end(b, ran, joints, states)


@pytest.mark.parametrize("how", ["max_cycles", "stop_in_mid_burst"])
@pytest.mark.parametrize("efforts_live", [False, True], ids=["c2", "c2_tipf"])
@pytest.mark.parametrize("n", SIZES)
def test_four_role_loop_ends_at_its_bound_or_in_mid_burst(Engine, n, efforts_live, how):
    """A run whose loop leaves by itself at max_cycles (= 40, inside the direct posts), and one that resident_end stops while a burst of several cycles is
    being run: all four wavefronts of every pair leave on the same iteration, and the state after the cycles that ran is the twin's after as many."""
    if how == "max_cycles":
        b, ran, released, joints, states = run_loop(Engine, n, efforts_live, BURSTS, stop_at=CYCLES, max_cycles=40)
        assert ran == released == 40
    else:
        b, ran, released, joints, states = run_loop(Engine, n, efforts_live, BURSTS, stop_at=12, max_cycles=CYCLES + 10)
        assert ran == released == 15   # what was released - the burst of cycles 8 .. 14 - and nothing more
    check_end(b, ran, joints, states)


@pytest.mark.parametrize("efforts_live", [False, True], ids=["c2", "c2_tipf"])
@pytest.mark.parametrize("n", [11, 21])
def test_three_role_form_of_the_same_build_is_byte_identical_too(Engine, monkeypatch, n, efforts_live):
    """SHC_RESIDENT_THREE_ROLE=1 (development, A/B runs): one helper wavefront runs what the two helpers of the four-role form share out."""
    monkeypatch.setenv("SHC_RESIDENT_THREE_ROLE", "1")
    b, ran, released, joints, states = run_loop(Engine, n, efforts_live, BURSTS, stop_at=CYCLES, max_cycles=CYCLES + 10)
    assert ran == released == CYCLES
    check_end(b, ran, joints, states)


_WHICH_BLOCK = """
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


@pytest.mark.parametrize("form", ["four_role", "three_role"])
@pytest.mark.parametrize("efforts_live", [False, True], ids=["c2", "c2_tipf"])
def test_which_helper_form_a_process_launches(tmp_path, efforts_live, form):
    """The forms are byte-identical by design, so the tests above cannot tell them apart: a fresh process logs the loop kernels it launches (SHC_KERNEL_LOG,
    "form legs joints features") - the helper form, "resident3", is the four-role one by default; SHC_RESIDENT_THREE_ROLE=1 keeps its predecessor with one
    helper wavefront, logged as "resident3_one_helper"."""
    log = tmp_path / "kernels.txt"
    env = dict(os.environ, SHC_KERNEL_LOG=str(log))
    env.pop("SHC_RESIDENT_TWO_ROLE", None)
    env.pop("SHC_RESIDENT_THREE_ROLE", None)
    if form == "three_role":
        env["SHC_RESIDENT_THREE_ROLE"] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", _WHICH_BLOCK.format(efforts=efforts_live)], cwd=root, env=env, check=True, timeout=120)
    features = 1 | 64 | (32 if efforts_live else 0)   # F_MANUAL | F_ODOM [| F_TIPF]
    loops = [line.split() for line in log.read_text().splitlines() if line.startswith("resident")]
    assert loops == [["resident3" if form == "four_role" else "resident3_one_helper", "6", "3", str(features)]], loops
