"""rcpIeee / divIeee (hpt_device.h) against the compiler's IEEE division, bit for bit (tests/cpp/exact_div_probe.hip).

The helpers replay the compiler's rcp + fma chain without v_div_scale / v_div_fmas' scaling / v_div_fixup, behind a guard on the exponents
(profiles/exact_div.md). The probe compares them with `1.0f / x` and `a / b` compiled in the same program:

  rcp_all      all 2^32 bit patterns; the lanes on the fast path must be exactly the guard range, 128 exponents x 2^24 patterns = 2^31
  div_edges    2048 x 2048 edge values (every exponent, mantissas 0, 1, 0x400000, 0x7FFFFF, both signs)
  div_random   2^28 seeded pairs of raw patterns
  div_inrange  2^28 seeded pairs inside the guard range: all of them on the fast path

No mismatch is allowed anywhere. The host mode of the same program checks the guard predicates against the documented ranges without a device.
"""
import json
import os
import subprocess

import pytest

import __graft_entry__ as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("exact_div") / "exact_div_probe")
    flags = [f for f in g.HIP_FLAGS if f != "-fPIC"]
    subprocess.check_call([g.HIPCC] + flags + ["-I" + g.CSRC, "-I" + os.path.join(ROOT, "include"),
                                               os.path.join(ROOT, "tests", "cpp", "exact_div_probe.hip"), "-o", exe])
    return exe


def lines(out):
    return {d["set"]: d for d in (json.loads(l) for l in out.splitlines() if l.startswith("{"))}


def test_guard_predicates_match_the_documented_ranges_on_the_host(probe):
    r = subprocess.run([probe, "--host"], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    d = lines(r.stdout)["host"]
    assert d["wrong"] == 0 and d["fast_build"] == 1


@pytest.mark.gpu
def test_helpers_equal_the_compilers_division_bit_for_bit(probe):
    r = subprocess.run(["timeout", "-k", "10", "120", probe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    d = lines(r.stdout)
    assert set(d) == {"rcp_all", "div_edges", "div_random", "div_inrange"}
    assert d["rcp_all"]["items"] == 1 << 32 and d["div_edges"]["items"] == 1 << 22
    assert d["div_random"]["items"] == d["div_inrange"]["items"] == 1 << 28
    for name, s in d.items():
        assert s["mismatches"] == 0, f"{name}: {s['mismatches']} mismatches, first operand words {s['first_bad']}"
    assert d["rcp_all"]["fast"] == 1 << 31                       # exponents 64 .. 191, every mantissa, both signs
    assert d["div_inrange"]["fast"] == 1 << 28                   # 100 % of the in-range set
    assert 0 < d["div_edges"]["fast"] < 1 << 22                  # (waves of the other two sets mix lanes in and out of range)
