"""The record layout behind BatchEngine.leg_state_msgs (no GPU): the numpy dtype follows params.LegStateMsg, which follows the header."""
import ctypes as C
import os
import re

import numpy as np

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.params import SHC_MAX_JOINTS, LegStateMsg

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "shc_batch.h")


def header_fields():
    """(name, doubles) of every member of struct shc_leg_state_msg, in declaration order."""
    text = open(HEADER).read()
    body = re.search(r"typedef struct shc_leg_state_msg \{(.*?)\} shc_leg_state_msg;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith("double "), decl
        for item in decl[len("double "):].split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\w+)\])?\s*", item)
            k = m.group(2)
            out.append((m.group(1), 1 if k is None else SHC_MAX_JOINTS if k == "SHC_MAX_JOINTS" else int(k)))
    return out


def test_ctypes_mirror_matches_the_header():
    fields = header_fields()
    assert [(n, C.sizeof(t) // 8) for n, t in LegStateMsg._fields_] == fields
    assert C.sizeof(LegStateMsg) == 512 == 8 * sum(k for _, k in fields)   # 64 doubles, no padding


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
    text = open(HEADER).read()
    for sym in ("shc_engine_get_leg_state_msgs", "shc_fleet_get_leg_state_msgs"):
        assert re.search(r"\bint " + sym + r"\(", text) and sym in engine.EXPORTED_SYMBOLS
        assert hasattr(engine.lib(), sym)
    assert engine.lib().shc_abi_version() == 6
