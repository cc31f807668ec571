"""The wavefront form of adaptive sampling without a GPU: its kernels are built into the library from a translation unit of their own, the switch is
an option (no new entry point: the export count stays), and the documents state it."""
import os
import re
import subprocess

from conftest import ROOT


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_kernels_are_built_and_no_entry_point_is_added():
    import __graft_entry__ as ge
    from hydracore3_amd import api
    unit = [u for u in ge.UNITS if u[0] == "wf_shade_adapt"]
    assert unit == [("wf_shade_adapt", "hpt_wavefront.hip", ["-DHPT_WF_INST=5"])]
    names = [u[0] for u in ge.UNITS]
    assert len(names) == len(set(names))
    api.load_library()
    syms = subprocess.run(["nm", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("wfInitCountsKernel", "wfCountsSummaryKernel"):
        assert re.search(r" [DTVW] _ZN3hpt\d+" + k + "E", syms), k
    # the three forward shade kernels an adaptive call can reach, ADAPT (the seventh flag) set: lean, every BSDF branch, moving instances
    for flags in ("Lb0ELb1ELb0ELb0ELb0ELb0ELb1E", "Lb0ELb0ELb0ELb0ELb0ELb0ELb1E", "Lb0ELb0ELb1ELb0ELb0ELb0ELb1E"):
        assert re.search(r" [DTVW] _ZN3hpt13wfShadeKernelI" + flags + "E", syms), flags
    assert len(set(re.findall(r" [DV] (_ZN3hpt13wfShadeKernelI(?:Lb[01]E){6}Lb1EEEv\S*)", syms))) == 3                       # ... and no other
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    n = len(re.findall(r" T hpt_\w+$", exported, flags=re.M))
    assert n == len(api.ABI) == 121, (n, len(api.ABI))


def test_option_is_documented_where_its_users_look():
    hdr = _read("include", "hydra_hip.h")
    m = re.search(r'"adaptive_wavefront"(.*?)\n \* Diagnostic switches', hdr, flags=re.S)
    assert m and "0xFFFFFF" in m.group(1) and "HPT_ERR_ARG" in m.group(1) and "0 (default)" in m.group(1)
    from hydracore3_amd.api import HipIntegrator
    assert "adaptive_wavefront" in HipIntegrator.set_option.__doc__
    design = _read("DESIGN.md")
    sec = design[design.index("### 2.13"):design.index("## 3. Oracle")]
    for word in ("**Wavefront form**", "wfInitCountsKernel", "wfCountsSummaryKernel", "adaptSampleLuminance", "0xFFFFFF", "profiles/adaptive_wavefront.md"):
        assert word in sec, word
    scope = design[design.index("## 7. Out of scope"):]
    assert "compacted to the active pixels" in scope
    assert os.path.exists(os.path.join(ROOT, "profiles", "adaptive_wavefront.md")) and os.path.exists(os.path.join(ROOT, "profiles", "adaptive_wavefront.py"))
    readme = _read("README.md")
    assert "test_adaptive_wavefront_gpu.py" in readme and "wfCountsSummaryKernel" in readme
