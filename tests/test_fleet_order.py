"""CPU: pick and place between a fleet caller's padded rows and a part's dense rows (csrc/shc_fleet_order.hpp), on their own.
tests/fleet_order_check.cpp includes that header alone (plain host C++, no HIP), is built here with the host compiler under AddressSanitizer and
UBSan, and runs as a child process: parts of the destination's geometry, with fewer legs, fewer joints and fewer of both; no row, one row,
several; ids that skip rows; words of 4 and 8 bytes, records of 64, 42, 20 and 4 words - against reference loops written in the program, in heap
blocks of exactly their size and a destination of 0xAB bytes, so that a stray word is a sanitizer report and an unwritten one a difference.
The program's own CHECKs name the line that fails."""
import os
import subprocess

from test_stage_arena import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fleet_order_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fleet_order_check")
    cxx = _host_compiler()
    # (static sanitizer runtimes where gcc has the archives: tests/test_stage_arena.py says why)
    archive = subprocess.run(cxx + ["-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()
    static = ["-static-libasan", "-static-libubsan"] if os.path.isabs(archive) and "clang" not in archive else []
    cmd = cxx + static + ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                              "-o", exe, os.path.join(HERE, "fleet_order_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, f"{' '.join(cmd)}\n{built.stderr[-4000:]}"
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and ran.stdout.strip().endswith("ok"), f"exit {ran.returncode}\n{ran.stdout[-4000:]}\n{ran.stderr[-4000:]}"
