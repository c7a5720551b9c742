"""csrc/account_scan_host.h for get_account_flow_matrix — the map builder and the bin adder on the
matrix's layout, as a node's host runs them — built as a stand-alone program with AddressSanitizer and
UndefinedBehaviorSanitizer and run on the CPU: tests/matrix_host_check.cpp feeds them hand-made and
random lists and bins and compares with a search and unsigned __int128 arithmetic.  Nothing is loaded
into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_maps_and_bin_adder_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    program = str(tmp_path / "matrix_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", program, os.path.join(HERE, "matrix_host_check.cpp")],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "matrix_host_check: 0 failures" in run.stdout
