"""The NCO's arithmetic on the CPU: quadrs_amd/csrc/qd_nco.h, the text every kernel compiles, built with the host compiler into
scripts/nco_host_check.cpp and held to __float128 there (table entries, the three-multiplication rotation, both orders, nco_mul_n
against nco_mul).  The program asserts the derived error budget of qd_nco.h (1.51e-15) below tests/util.py's NCO_ABS_ERR, the
multiplier against that budget less the device-libm term, and the rotation's own roundings against 3.9e-16; figures of one run:
first order 4.9e-16, second order 4.8e-16, rotation 3.5e-16."""
import os
import subprocess

import pytest

from util import NCO_ABS_ERR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nco") / "nco_host_check")
    src = os.path.join(ROOT, "scripts", "nco_host_check.cpp")
    r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, src, "-lquadmath"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_header_is_host_clean(tmp_path):
    """qd_nco.h alone is plain C++17: no HIP type, nothing of the other kernel headers"""
    tu = tmp_path / "only_nco.cpp"
    tu.write_text('#include "qd_nco.h"\nstatic_assert(sizeof(qd::RowBase) == 32 && sizeof(qd::LaneEntry) == 24 && sizeof(qd::LaneRot) == 32, "layout");\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "quadrs_amd", "csrc"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "quadrs_amd", "csrc", "qd_nco.h")).read()
    assert "float2" not in text and "double2" not in text and "hip_runtime" not in text


def test_rotation_and_multiplier_against_float128(host_check):
    r = subprocess.run([host_check, repr(NCO_ABS_ERR)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "nco_host_check: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
    assert "derived total 1.512e-15" in r.stdout


def test_a_dropped_rounding_guard_fails_the_rotation_bound(host_check):
    """mutation: the row entry's cs as an f32-rounded sum; the 3.9e-16 assertion must catch it"""
    r = subprocess.run([host_check, repr(NCO_ABS_ERR), "--mutate", "cs32"], capture_output=True, text=True)
    assert r.returncode == 1 and "FAILED rotation rounding" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])


def test_derived_total_must_lie_below_the_rule(host_check):
    """the program refuses a rule at or below its derived total"""
    r = subprocess.run([host_check, "1.5e-15"], capture_output=True, text=True)
    assert r.returncode == 1 and "derived total not below the rule" in r.stdout, r.stdout[-2000:]
