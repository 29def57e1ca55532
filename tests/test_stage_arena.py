"""CPU: StageArena, the allocator under every host-array call (csrc/shc_stage.hpp), on its own.  tests/stage_arena_check.cpp includes the arena
part of the header alone (plain host C++, no HIP), is built here with the host compiler under AddressSanitizer and UBSan, and runs as a child
process: alignment of every take, no overlap, nothing past the capacity, refusals that leave the cursor alone (count * size overflow among them),
zero-size takes, exact release under three levels of nesting and reuse after a release.  The program's own CHECKs name the line that fails."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_compiler():
    for cmd in (["g++"], ["c++"], ["clang++"], [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]):
        if shutil.which(cmd[0]):
            return cmd
    raise FileNotFoundError("no host C++ compiler (g++, c++, clang++ or hipcc)")


def test_stage_arena_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "stage_arena_check")
    cxx = _host_compiler()
    # gcc links the sanitizer runtimes dynamically, and ASan then insists on being the first library of the process: link them statically where the
    # archives exist, so that the program also runs where the environment preloads a library of its own (clang links them statically anyway)
    archive = subprocess.run(cxx + ["-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()
    static = ["-static-libasan", "-static-libubsan"] if os.path.isabs(archive) and "clang" not in archive else []
    cmd = cxx + static + ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                              "-o", exe, os.path.join(HERE, "stage_arena_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, f"{' '.join(cmd)}\n{built.stderr[-4000:]}"
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and ran.stdout.strip().endswith("ok"), f"exit {ran.returncode}\n{ran.stdout[-4000:]}\n{ran.stderr[-4000:]}"
