"""csrc/account_scan_host.h — the index and the bin adder a node's host runs for the account-set scan's
calls — built as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer and run on
the CPU: tests/account_scan_host_check.cpp feeds them hand-made and random bins and ids and compares
with unsigned __int128 arithmetic.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_index_and_bin_adder_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    program = str(tmp_path / "account_scan_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-o", program, os.path.join(HERE, "account_scan_host_check.cpp")],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "account_scan_host_check: 0 failures" in run.stdout
