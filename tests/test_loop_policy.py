"""CPU: the registration loop's host policy (csrc/loop_policy.h: the chunk schedule, the halo decision, the re-location
arming, the search skip's gate, the form of a search launch) rule by rule -- tests/cpp/test_loop_policy.cpp, a
stand-alone program that includes nothing but that header, built with AddressSanitizer and UBSan and run directly."""
import os
import subprocess

from conftest import ROOT


def test_every_rule_of_the_loop_policy(tmp_path):
    exe = str(tmp_path / "test_loop_policy")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "cupoch_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_loop_policy.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "ok"
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
