"""GPU (-m gpu): the layouts the one reader of array arguments (syropod_highlevel_controller_amd/arrays.py) newly accepts - a dimension of extent
1 whose stride is not the dense one - reach the library as the contiguous array of their shape does.  torch itself reports no strides for
such a tensor, so a wrapper publishes a tensor's pointer with strides of its own choosing.  Everything else about these calls:
tests/test_gpu_actions.py, tests/test_gpu_observations.py; every other layout, without a GPU: tests/test_array_args.py."""
import numpy as np
import pytest

from syropod_highlevel_controller_amd.engine import BatchEngine, action_columns, device_count
from syropod_highlevel_controller_amd.fleet import MixedFleet
from test_gpu_actions import action_values, joint_bits
from test_gpu_fleet_device_io import views
from test_gpu_observations import drive
from test_gpu_resident import config3_params, state_bytes

pytestmark = pytest.mark.gpu

FIELDS = ("linear_xy", "angular", "imu_orientation", "imu_angular_velocity", "tip_force")
SENTINEL = -7.0


class Strided:
    """The memory of a torch tensor under a shape and byte strides of the caller's choosing."""

    def __init__(self, tensor, shape, strides):
        self.tensor = tensor   # (keeps the memory alive)
        self.__cuda_array_interface__ = dict(tensor.__cuda_array_interface__, shape=tuple(shape), strides=tuple(strides))


def one_row(seed=5):
    """(the (1, A) float32 tensor, the same memory presented with strides[0] = 7 bytes)"""
    import torch
    rows = action_values(seed, 1, FIELDS, 6, 3, 6, 3)
    assert rows.shape == (1, action_columns(FIELDS, 6, 3)[1])
    tensor = torch.from_numpy(rows).to(torch.float32).cuda()
    torch.cuda.synchronize()   # the engines run on streams of their own: the tensor is complete before a call
    assert tensor.__cuda_array_interface__["strides"] is None
    return tensor, Strided(tensor, tensor.shape, (7, 4))


def a_column():
    """(the (3, 8) float32 tensor full of SENTINEL, its column 3 presented as (3, 1) with the strides (32, 8), the plain view big[:, 3:4])"""
    import torch
    big = torch.full((3, 8), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    plain = big[:, 3:4]
    return big, Strided(plain, (3, 1), (32, 8)), plain


def assert_the_column_alone_was_written(big, expected, what):
    import torch
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert np.array_equal(got[:, 3], expected), what
    assert (np.delete(got, 3, axis=1) == SENTINEL).all(), f"{what}: another column was written"


def need_gpu():
    if device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")


@pytest.fixture(scope="module")
def one_robot():
    """Engines of 1 robot 3 cycles after set_actions: {fed the row with strides[0] = 7 bytes, fed it contiguously, never fed}: (joints, state records)"""
    need_gpu()
    p = config3_params()
    engines = {name: BatchEngine(p, 1) for name in ("strided", "contiguous", "never")}
    try:
        for e in engines.values():
            drive(e, p, 3)
        assert len({state_bytes(e) for e in engines.values()}) == 1
        tensor, strided = one_row()
        engines["strided"].set_actions(strided, FIELDS)
        engines["contiguous"].set_actions(tensor, FIELDS)
        for e in engines.values():
            e.step(3)
            e.synchronize()
        return {name: (joint_bits(e), state_bytes(e)) for name, e in engines.items()}
    finally:
        for e in engines.values():
            e.close()


@pytest.fixture(scope="module")
def three_robots():
    """An engine of 3 robots: (the (3, 8) tensor whose column 3 was filled as (3, 1) with strides (32, 8), the one filled through big[:, 3:4],
    body_state()'s walk states)"""
    need_gpu()
    p = config3_params()
    eng = BatchEngine(p, 3)
    try:
        drive(eng, p, 4)   # (robot 0 stands, the others walk: the column is not one value)
        big, strided, _ = a_column()
        eng.observations(("walk_state",), out=strided)
        other, _, plain = a_column()
        eng.observations(("walk_state",), out=plain)
        eng.synchronize()
        return big, other, eng.body_state()[2].astype(np.float32)
    finally:
        eng.close()


def test_one_robot_takes_a_row_with_an_odd_stride(one_robot):
    assert one_robot["strided"][0] == one_robot["contiguous"][0], "the joints differ 3 cycles later"
    assert one_robot["strided"][1] == one_robot["contiguous"][1], "the state records differ 3 cycles later"
    assert one_robot["never"][0] != one_robot["strided"][0], "the actions changed nothing: the comparison above shows nothing"


def test_three_robots_fill_a_column_presented_with_both_strides(three_robots):
    big, other, walk_state = three_robots
    assert len(set(walk_state)) > 1
    assert_the_column_alone_was_written(other, walk_state, "the plain view")
    assert_the_column_alone_was_written(big, other.cpu().numpy()[:, 3], "the column with strides (32, 8)")


def test_the_same_two_layouts_through_a_fleet_of_one_part(one_robot, three_robots):
    need_gpu()
    p = config3_params()
    one, three = MixedFleet([p], np.zeros(1, dtype=np.int32), (0,)), MixedFleet([p], np.zeros(3, dtype=np.int32), (0,))
    try:
        assert (one.max_legs, one.max_dof, len(one.parts())) == (6, 3, 1)
        (part, _), = views(one)
        drive(part, p, 3)
        _, strided = one_row()
        one.set_actions(strided, FIELDS)
        one.step(3)
        one.synchronize()
        assert (joint_bits(part), state_bytes(part)) == one_robot["contiguous"], "the fleet's one robot is not where the engine's is"
        (part, ids), = views(three)
        assert list(ids) == [0, 1, 2]
        drive(part, p, 4)
        big, strided, _ = a_column()
        three.observations(strided, ("walk_state",))
        three.synchronize()
        assert_the_column_alone_was_written(big, three_robots[2], "the fleet's column with strides (32, 8)")
    finally:
        one.close(), three.close()
