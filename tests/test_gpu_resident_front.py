"""GPU (-m gpu): the three-role resident 6 x 3 loop with the front of updateWalk - getLimit and the desired body velocities - on the helper wavefront
(shc_resident2_kernel<6, 3, F_C2 [| F_TIPF], true>: walk_velocity_front on the helper, cycle_front<..., FRONT_HERE = false> on the walker) against
set_* + shc_engine_step(1) on a twin engine, byte for byte: every cycle's q / qd from the output ring, the complete state record and the odometry
after resident_end - and the same loop with SHC_RESIDENT_TWO_ROLE=1 (the two-role form of the same build, front on the walker).

What the inputs reach: a fresh velocity command through ring posts, one direct post from bound arrays and bare publishes in between (the helper takes a
fresh command from its source itself and a held one from the tile); a stretch of zero command (all four walk states: the STOPPING branch of the shaping,
the robot word stored behind the front's flag); commands outside the unit disc and jumps beyond the acceleration cap; both velocity input modes; a
command whose direction turns, so that stride bearings cross 45-degree sector edges (the bracket memo misses) and a held stretch (it hits).
Batch sizes: 1 robot, 10 (one full wave), 11 (a partial second pair), 21 (a second workgroup whose second pair is inactive).
"""
import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params

pytestmark = pytest.mark.gpu

SEED = 7              # chosen on the CPU oracle (tests/oracle_lib.OracleBatch through twin_records): both preconditions hold for every case below
CYCLES = 64
HISTORY = 45          # ordinary launches before the loop starts: the robots are walking when it does
STOP = range(4, 30)   # a stretch of zero command
HELD = range(49, 55)  # a stretch of bare publishes while the robots walk
DIRECT = 37
WS_STARTING, WS_MOVING, WS_STOPPING, WS_STOPPED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def Engine():
    from syropod_highlevel_controller_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    return engine.BatchEngine


def params(mode):
    p = default_hexapod_params("tripod")
    p.step_frequency = 5.0   # a 24-iteration step cycle: STOPPING -> STOPPED -> STARTING -> MOVING fits the run
    p.velocity_input_mode = mode
    return p


def state_bytes(eng):
    return bytes(memoryview(eng.get_state()).cast("B"))


def plan(n, efforts_live, mode):
    """What every cycle of the run receives (the same for the twin engine and the loop).  post: the cycle carries inputs (else a bare publish: held)."""
    rng = np.random.default_rng(SEED + 1000 * n + 10 * int(efforts_live) + mode)
    phase, turn = rng.uniform(0, 2 * np.pi, n), rng.uniform(-1.3, 1.3, n)   # (|angular input| above 1: the clamp)
    cyc = []
    for c in range(CYCLES):
        r = 1.7 if c % 9 == 5 else (0.03 if c % 11 == 7 else 0.6)   # outside the unit disc / a jump far beyond the acceleration cap, both ways
        th = 0.45 * c + phase                                       # the command's direction turns: stride bearings cross sector edges
        lin = r * np.stack([np.cos(th), np.sin(th)], axis=1)
        ang = turn * (0.4 + 0.6 * np.sin(0.23 * c + np.arange(n)))
        if mode == 1:                                               # real units: around the speed limits, below and above them
            lin, ang = lin * 0.2, ang * 0.5
        if c in STOP:
            lin, ang = np.zeros((n, 2)), np.zeros(n)
        bare = (c % 5 == 2 or c in HELD) and c != DIRECT
        d = {"post": not bare, "velocity": (lin, ang), "pose_input": None, "pose_reset_mode": None, "joint_effort": None, "direct": c == DIRECT}
        if c in (33, 41):     # joystick body posing mid-run ...
            d["pose_input"] = (rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3)))
        if c == 46:           # ... a reset mode, and its release
            d["pose_reset_mode"] = rng.integers(1, 6, n).astype(np.int32)
        if c == 55:
            d["pose_reset_mode"] = np.zeros(n, dtype=np.int32)
        if efforts_live and (c % 7 == 3 or c == DIRECT) and not bare:
            d["joint_effort"] = rng.normal(0, 0.5, (n, 18))
        assert bare <= all(d[k] is None for k in ("pose_input", "pose_reset_mode", "joint_effort"))
        cyc.append(d)
    return cyc, rng.normal(0, 0.5, (n, 18))


def prepare(make, n, efforts_live, mode, e0, first):
    e = make(params(mode), n)
    e.set_pose_input(np.zeros((n, 3)), np.zeros((n, 3)))   # (the manual-pose group of the state is live from the first pose input on)
    if efforts_live:
        e.set_joint_effort(e0)
    e.set_velocity(*first)
    e.step(HISTORY)
    return e


def bearing_bracket(y, x):
    """WalkController::getLimit's bracket as the kernels find it (shc_cycle.hpp, bearing_bracket): the 45-degree sector of the direction turned by half a degree."""
    kc, ks = 0.99996192306417128874, 0.0087265354983739347
    xr, yr = kc * x - ks * y, ks * x + kc * y
    ax, ay = np.abs(xr), np.abs(yr)
    upper = (yr > 0.0) | ((yr == 0.0) & (xr > 0.0))
    up = np.where(xr > 0.0, np.where(ay < ax, 0, 1), np.where(ay > ax, 2, 3))
    lo = np.where(xr < 0.0, np.where(ay < ax, 4, 5), np.where(ay > ax, 6, 7))
    return np.where((x == 0.0) & (y == 0.0), 0, np.where(upper, up, lo))


def twin_records(a, cyc, on_cycle=None):
    """Runs the plan on `a` (an engine or the CPU oracle) cycle by cycle.  Returns the walk states met, and per cycle whether some leg's bearing bracket differs
    from the previous cycle's and whether the command in force is non-zero.
    An approximation of the loop's memo, good enough for a precondition: this looks at the whole batch and at the previous CYCLE's brackets; the kernel keeps one
    memo per wavefront (10 robots) and compares with the brackets of that wavefront's last MISS.  For one wave (n <= 10) "some leg changed" is a miss and "none
    changed" right after a miss is a hit; for n = 11 and 21 (two and three waves) it shows that the batch met both, not that every wave did."""
    walk, brackets, moving = set(), [], []
    for c, d in enumerate(cyc):
        if d["post"]:
            a.set_velocity(*d["velocity"])
            held = d["velocity"]
            if d["pose_input"] is not None:
                a.set_pose_input(*d["pose_input"])
            if d["pose_reset_mode"] is not None:
                a.set_pose_reset_mode(d["pose_reset_mode"])
            if d["joint_effort"] is not None:
                a.set_joint_effort(d["joint_effort"])
        elif c == 0:
            held = d["velocity"]
        tip = a.leg_state()["walker_tip"]   # the tips the previous cycle left: what getLimit of this cycle reads
        (lin, ang) = held
        brackets.append(bearing_bracket(lin[:, 1, None] + ang[:, None] * tip[:, :, 0], lin[:, 0, None] - ang[:, None] * tip[:, :, 1]))
        moving.append(bool(np.any(lin != 0.0) or np.any(ang != 0.0)))
        a.step(1)
        walk |= set(int(w) for w in a.body_state()[2])
        if on_cycle is not None:
            on_cycle(a)
    changed = [bool((brackets[c] != brackets[c - 1]).any()) for c in range(1, len(cyc))]
    return walk, changed, moving[1:]


def check_preconditions(walk, changed, moving):
    # the inputs do what they are there for: the general walk state machine with its stop predicates ...
    assert walk == {WS_STARTING, WS_MOVING, WS_STOPPING, WS_STOPPED}, walk
    # ... and the bracket memo of the loop both misses (some leg's bracket differs from the previous cycle's) and hits (none does), the latter also under a command
    assert any(changed), "no cycle in which a leg changes its bearing bracket"
    assert not all(changed), "no cycle in which every leg keeps its bearing bracket"
    assert any(m and not ch for ch, m in zip(changed, moving)), "every leg keeps its bracket only while the command is zero"


_reference = {}


def reference(Engine, n, efforts_live, mode):
    """The twin engine: set_* + shc_engine_step(1) per cycle; computed once per case, shared by the tests, never changed."""
    key = (n, efforts_live, mode)
    if key not in _reference:
        cyc, e0 = plan(n, efforts_live, mode)
        a = prepare(Engine, n, efforts_live, mode, e0, cyc[0]["velocity"])
        joints, states = [], [None]   # states[c]: (state record, odometry) after c cycles

        def record(a):
            joints.append(a.joints())
            states.append((state_bytes(a), a.odometry().copy()))
        walk, changed, moving = twin_records(a, cyc, record)
        a.close()
        check_preconditions(walk, changed, moving)
        _reference[key] = (cyc, e0, joints, states)
    return _reference[key]


def bursts_of(cyc, total):
    """(first cycle, length) of every release: publish(k) bursts mixed with single ticks.  Posts fill the next unposted cycle, so a burst is posted cycles
    followed by bare ones; the direct post is a release of its own."""
    sizes, out, c, i = [1, 1, 5, 1, 7, 2, 1, 6, 3, 1, 7, 1, 4], [], 0, 0
    while c < total:
        k, j = min(sizes[i % len(sizes)], total - c), 1
        i += 1
        while j < k and not cyc[c].get("direct") and not cyc[c + j]["direct"] and not (cyc[c + j]["post"] and not cyc[c + j - 1]["post"]):
            j += 1
        out.append((c, j))
        c += j
    return out


def run_loop(Engine, n, efforts_live, mode, stop_at, max_cycles):
    """The same cycles through one resident launch, each release waited for (so that the loop idles in between); ended by resident_end right behind the release
    of the burst that reaches stop_at (the loop stops once it has run what was released), or by itself at max_cycles.  Returns (engine, cycles run, cycles
    released, the twin's joints, the twin's states)."""
    import torch
    cyc, e0, joints, states = reference(Engine, n, efforts_live, mode)
    b = prepare(Engine, n, efforts_live, mode, e0, cyc[0]["velocity"])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    lin_d, ang_d = dev(cyc[DIRECT]["velocity"][0]), dev(cyc[DIRECT]["velocity"][1])
    eff_d = dev(cyc[DIRECT]["joint_effort"] if efforts_live else np.zeros((n, 18)))
    torch.cuda.current_stream().synchronize()
    b.resident_bind_inputs(0, velocity=(lin_d.data_ptr(), ang_d.data_ptr()), joint_effort=eff_d.data_ptr() if efforts_live else None)
    b.resident_begin(ring_depth=8, max_cycles=max_cycles)
    total = min(CYCLES, max_cycles)
    for c, k in bursts_of(cyc, total):
        for d in cyc[c:c + k]:
            if d["direct"]:
                kw = {"velocity": True}
                if efforts_live:
                    kw["joint_effort"] = True
                assert b.resident_post(direct=0, **kw) == c   # (released at once)
            elif d["post"]:
                b.resident_post(**{key: d[key] for key in ("velocity", "pose_input", "pose_reset_mode", "joint_effort") if d[key] is not None})
        if not cyc[c]["direct"]:
            b.resident_publish(k)
        if c < stop_at <= c + k and stop_at < total:   # resident_end in mid-burst
            return b, b.resident_end(), c + k, joints, states
        b.resident_wait(c + k)
        for cc in range(c, c + k):
            q, qd = b.resident_joints(cc)
            assert np.array_equal(q, joints[cc][0]) and np.array_equal(qd, joints[cc][1]), f"cycle {cc}"
    return b, b.resident_end(), total, joints, states


@pytest.mark.parametrize("form", ["helper", "two_role"])
@pytest.mark.parametrize("mode", [0, 1], ids=["throttle", "real"])
@pytest.mark.parametrize("efforts_live", [False, True], ids=["c2", "c2_tipf"])
@pytest.mark.parametrize("n", [1, 10, 11, 21])
def test_loop_with_the_front_on_the_helper_is_byte_identical_to_single_cycle_launches(Engine, monkeypatch, n, efforts_live, mode, form):
    if form == "two_role":
        monkeypatch.setenv("SHC_RESIDENT_TWO_ROLE", "1")
    else:
        monkeypatch.delenv("SHC_RESIDENT_TWO_ROLE", raising=False)
    b, ran, released, joints, states = run_loop(Engine, n, efforts_live, mode, stop_at=CYCLES, max_cycles=CYCLES + 10)
    assert ran == released == CYCLES
    assert state_bytes(b) == states[CYCLES][0]
    assert np.array_equal(b.odometry(), states[CYCLES][1]) and np.abs(states[CYCLES][1][:, :2]).max() > 1e-3
    b.close()


@pytest.mark.parametrize("how", ["max_cycles", "end_in_mid_burst"])
def test_loop_with_the_front_on_the_helper_ends_at_its_bound_or_in_mid_burst(Engine, monkeypatch, how):
    """A run whose loop leaves by itself at max_cycles (= 40), and one that resident_end stops while a burst of several cycles is being run:
    the state after the cycles that ran - the velocities the helper left in the tile among it - is the twin's after as many."""
    monkeypatch.delenv("SHC_RESIDENT_TWO_ROLE", raising=False)
    n = 21
    if how == "max_cycles":
        b, ran, released, joints, states = run_loop(Engine, n, True, 1, stop_at=CYCLES, max_cycles=40)
        assert ran == released == 40
    else:
        b, ran, released, joints, states = run_loop(Engine, n, True, 0, stop_at=41, max_cycles=CYCLES + 10)
        assert ran == released == 43   # what was released - the burst of cycles 39 .. 42 - and nothing more
    q, qd = b.joints()
    assert np.array_equal(q, joints[ran - 1][0]) and np.array_equal(qd, joints[ran - 1][1])
    assert state_bytes(b) == states[ran][0] and np.array_equal(b.odometry(), states[ran][1])
    b.close()
