"""lattigo_amd/csrc/ks_route.h on the CPU: tests/cpp/ks_route_test.cpp enumerates every combination of the facts a key switch's
launch route depends on, asserts the invariants the launch code relies on and pins one route per row of DESIGN.md section 4.
The header is host-only, so the program needs neither the library nor a device; it is built with g++ -Wall -Wextra, and once more
under the address and undefined-behaviour sanitizers (which cover ks_route.h only: nothing loaded into Python is sanitized)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("target", ["ks_route_test", "ks_route_test_san"])
def test_route_invariants_and_pinned_routes(target):
    r = subprocess.run(["make", "-C", CPP, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([os.path.join(CPP, target)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout and " 0 failed" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
