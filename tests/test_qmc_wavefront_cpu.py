"""The wavefront form of PathTraceBlockQMC without a GPU: its kernels are built into the library from translation units of their own, the switch is
an option (no new entry point: the export count stays), and the documents state it."""
import os
import re
import subprocess

from conftest import ROOT

NEW_UNITS = [("wf_shade_qmc", "hpt_wavefront.hip", ["-DHPT_WF_INST=6"]), ("wf_shade_qmc_motion", "hpt_wavefront.hip", ["-DHPT_WF_INST=7"])]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_units_are_appended_and_their_names_are_unique():
    import __graft_entry__ as ge
    assert ge.UNITS[-len(NEW_UNITS):] == NEW_UNITS                           # appended: the earlier entries keep their places
    names = [u[0] for u in ge.UNITS]
    assert len(names) == len(set(names))
    assert names.index("adaptive_spectral_wide4") == len(names) - len(NEW_UNITS) - 1


def test_kernels_are_built_and_no_entry_point_is_added():
    from hydracore3_amd import api
    api.load_library()
    syms = subprocess.run(["nm", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" [DTVW] _ZN3hpt\d+wfInitQmcKernelE", syms)
    for motion in (0, 1):                                                  # every BSDF branch; moving instances
        assert re.search(r" [DV] _ZN3hpt\d+wfShadeQmcKernelILb%dEEEv" % motion, syms), motion
    assert len(set(re.findall(r" [DV] (_ZN3hpt\d+wfShadeQmcKernelI\S*)", syms))) == 2      # ... and no other
    # the kernels that were there keep their names: no flag was added to wfShadeKernel or wfShadeSpecKernel
    assert len(set(re.findall(r" [DV] (_ZN3hpt13wfShadeKernelI(?:Lb[01]E){7}EEv\S*)", syms))) == 11
    assert len(set(re.findall(r" [DV] (_ZN3hpt\d+wfShadeSpecKernelILi\dELb[01]EEEv\S*)", syms))) == 6
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    n = len(re.findall(r" T hpt_\w+$", exported, flags=re.M))
    assert n == len(api.ABI) == 121, (n, len(api.ABI))


def test_option_is_documented_where_its_users_look():
    hdr = _read("include", "hydra_hip.h")
    m = re.search(r'\n \*   "qmc_wavefront"(.*?)\n \* Which schedule serves adaptive sampling', hdr, flags=re.S)
    assert m, "include/hydra_hip.h does not list the option before the adaptive options"
    for word in ("0 (default)", "HPT_ERR_ARG", "0xFFFFFF", "thin films", "sweep", "instrumented", "hpt_get_last_launch"):
        assert word in m.group(1), word
    assert "Megakernel schedule only. hpt_get_execution_time(\"PathTraceBlockQMC\")" not in hdr
    from hydracore3_amd.api import HipIntegrator
    assert "qmc_wavefront" in HipIntegrator.set_option.__doc__
    design = _read("DESIGN.md")
    sec = design[design.index("### 2.8"):design.index("### 2.9")]
    for word in ("**Wavefront form**", "qmc_wavefront", "wfShadeQmcKernel", "wfInitQmcKernel", "0xFFFFFF", "profiles/qmc_wavefront.md"):
        assert word in sec, word
    scope = design[design.index("## 7. Out of scope"):]
    assert "QMC under the block-local and wavefront schedules is not built" not in scope and "qmc_wavefront" in scope
    readme = _read("README.md")
    for word in ("qmc_wavefront", "test_qmc_wavefront_gpu.py", "test_qmc_wavefront_cpu.py", "wfShadeQmcKernel"):
        assert word in readme, word


def test_profile_and_its_script_exist():
    prof = _read("profiles", "qmc_wavefront.md")
    for word in ("VGPR", "scratch", "LDS", "unchanged", "Mpaths/s"):
        assert word in prof, word
    assert os.path.exists(os.path.join(ROOT, "profiles", "qmc_wavefront.py"))
