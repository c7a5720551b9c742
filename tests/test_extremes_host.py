"""csrc/extreme_op.h — get_account_balance_extremes' operator, the one function the kernel, the emit's
fold and the host's exact path compose segments with — built as a stand-alone program with
AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU: tests/extremes_host_check.cpp checks
its identity, associativity, tie rule, signed 192-bit compare and carries against a walk in __int128
limbs, folding random sequences split at every cut point.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_operator_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    program = str(tmp_path / "extremes_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", program, os.path.join(HERE, "extremes_host_check.cpp")],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "extremes_host_check: 0 failures" in run.stdout
