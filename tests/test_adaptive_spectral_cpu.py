"""Adaptive sampling under m_spectral_mode without a GPU: the ADAPT kernels of hpt_spectral.hip are built into the library from translation units
of their own, the switch is an option (no new entry point: the export count stays), and the documents state it."""
import os
import re
import subprocess

from conftest import ROOT

NEW_UNITS = [("adaptive_spectral", "hpt_spectral.hip", ["-DHPT_SPEC_INST=13"]), ("adaptive_spectral_gltf", "hpt_spectral.hip", ["-DHPT_SPEC_INST=14"]),
             ("adaptive_spectral_wide", "hpt_spectral.hip", ["-DHPT_SPEC_INST=15"]), ("adaptive_spectral_wide4", "hpt_spectral.hip", ["-DHPT_SPEC_INST=16"])]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_units_are_listed_and_their_names_are_unique():
    import __graft_entry__ as ge
    for unit in NEW_UNITS:
        assert [u for u in ge.UNITS if u[0] == unit[0]] == [unit], unit[0]
    names = [u[0] for u in ge.UNITS]
    assert len(names) == len(set(names))
    assert names.index("wf_shade_adapt") < min(names.index(u[0]) for u in NEW_UNITS)          # appended: the earlier entries keep their places


def test_adapt_kernels_are_built_and_no_entry_point_is_added():
    from hydracore3_amd import api
    api.load_library()
    syms = subprocess.run(["nm", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    for scope in (0, 1, 2, 3):                                             # DEEP x FLAT, SWEEP, and the four moving-instance variants: nine per scope, ADAPT (the last flag) set
        found = set(re.findall(r" [DV] (_ZN3hpt\d+pathTraceSpectralKernelI(?:Lb[01]E){4}Li%dELb1EEEv\S*)" % scope, syms))
        assert len(found) == 9, (scope, sorted(found))
        plain = set(re.findall(r" [DV] (_ZN3hpt\d+pathTraceSpectralKernelI(?:Lb[01]E){4}Li%dELb0EEEv\S*)" % scope, syms))
        assert len(plain) == 9, (scope, sorted(plain))
    for scope in (1, 2, 3):                                                # the wavefront schedule has no scope-0 shade kernel: scope 0 runs scope 1's
        assert re.search(r" [DV] _ZN3hpt\d+wfShadeSpecKernelILi%dELb1EEEv" % scope, syms), scope
        assert re.search(r" [DV] _ZN3hpt\d+wfShadeSpecKernelILi%dELb0EEEv" % scope, syms), scope
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    n = len(re.findall(r" T hpt_\w+$", exported, flags=re.M))
    assert n == len(api.ABI) == 121, (n, len(api.ABI))


def test_option_is_documented_where_its_users_look():
    hdr = _read("include", "hydra_hip.h")
    m = re.search(r'\n \*   "adaptive_spectral"(.*?)\n \* Diagnostic switches', hdr, flags=re.S)
    assert m, "include/hydra_hip.h does not list the option"
    for word in ("0 (default)", "HPT_ERR_UNSUPPORTED", "HPT_ERR_ARG", "channels > 4", "adaptive_wavefront", "thin film"):
        assert word in m.group(1), word
    assert hdr.index('"adaptive_wavefront"  0 (default)') < hdr.index('"adaptive_spectral"  0 (default)')
    from hydracore3_amd.api import HipIntegrator
    assert "adaptive_spectral" in HipIntegrator.set_option.__doc__
    design = _read("DESIGN.md")
    sec = design[design.index("### 2.13"):design.index("## 3. Oracle")]
    for word in ("**Spectral form**", "adaptive_spectral", "pathTraceSpectralKernel", "wfShadeSpecKernel", "adaptSampleLuminance", "profiles/adaptive_spectral.md"):
        assert word in sec, word
    scope = design[design.index("## 7. Out of scope"):]
    assert "adaptive_spectral" in scope and "RGB scenes with thin films" in scope
    readme = _read("README.md")
    for word in ("adaptive_spectral", "test_adaptive_spectral_gpu.py", "test_adaptive_spectral_cpu.py"):
        assert word in readme, word


def test_profile_and_its_script_exist():
    prof = _read("profiles", "adaptive_spectral.md")
    for word in ("VGPR", "scratch", "LDS", "unchanged"):
        assert word in prof, word
    assert os.path.exists(os.path.join(ROOT, "profiles", "adaptive_spectral.py"))
