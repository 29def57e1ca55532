"""The record layout behind BatchEngine.leg_state_msgs (no GPU): the numpy dtype follows params.LegStateMsg, which follows the header."""
import ctypes as C

import numpy as np

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.params import LegStateMsg


def test_numpy_dtype_follows_the_ctypes_mirror():
    dt = engine.LEG_STATE_MSG_DTYPE
    assert dt.itemsize == 512 == C.sizeof(LegStateMsg)
    assert list(dt.names) == [n for n, _ in LegStateMsg._fields_]
    for name, typ in LegStateMsg._fields_:
        sub, offset = dt.fields[name][:2]
        assert offset == getattr(LegStateMsg, name).offset, name
        assert sub.base == np.float64 and sub.itemsize == C.sizeof(typ), name
    rec = LegStateMsg()
    rec.auto_pose[3], rec.virtual_stiffness, rec.joint_efforts[5] = 1.0, 2.5, -3.0
    a = np.frombuffer(bytes(rec), dtype=dt)
    assert a["auto_pose"][0, 3] == 1.0 and a["virtual_stiffness"][0] == 2.5 and a["joint_efforts"][0, 5] == -3.0


def test_new_entry_points_are_declared_and_exported():
    for sym in ("shc_engine_get_leg_state_msgs", "shc_fleet_get_leg_state_msgs"):
        assert engine.HEADER.functions[sym][0] == "int" and sym in engine.EXPORTED_SYMBOLS
        assert hasattr(engine.lib(), sym)
    assert engine.lib().shc_abi_version() == 6
