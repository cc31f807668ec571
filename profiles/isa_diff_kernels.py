#!/usr/bin/env python3
"""Are the kernels two builds have in common the same code? profiles/isa_diff.sh compares whole translation units; this compares kernel by kernel,
for a change that ADDS kernels to a unit and a template flag to others (every mangled name then carries one more `false`).

  python profiles/isa_diff_kernels.py <build dir A> <build dir B> unit [unit ...]   e.g.  ... ../parent/hydracore3_amd/build hydracore3_amd/build wf_shade wf_trace

The gfx950 code object of each unit is extracted (llvm-objcopy, clang-offload-bundler) and disassembled (llvm-objdump -d); the text is cut at the
function labels, addresses and symbol references are removed, and a function of A is looked up in B under its own name and under that name with
one more `Lb0E` before the closing `E` of its template arguments. Prints one line per function of A (same / DIFFERENT / missing) and the names B
has beyond them; exit status 1 unless every function of A is in B with the same instructions."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM", "/opt/rocm/llvm/bin")


def functions(obj, tmp):
    fat, co = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:$", line)
        if m:
            name = m.group(1); out[name] = []
        elif name is not None and line.strip():
            line = re.sub(r"<[^>]*>", "", line)                 # symbol references
            line = re.sub(r"^\s*[0-9a-f]+:", "", line)          # (never present with --no-show-raw-insn's layout; kept for either)
            line = re.sub(r"//.*", "", line).strip()            # the address comment
            if line:
                out[name].append(line)
    return out


def main():
    a_dir, b_dir, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    rc = 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            fa, fb = functions(os.path.join(a_dir, u + ".o"), tmp), functions(os.path.join(b_dir, u + ".o"), tmp)
            seen = set()
            for name, body in sorted(fa.items()):
                twin = name if name in fb else re.sub(r"EEEv", "ELb0EEEv", name, count=1)   # ...<last argument>E, the arguments' E, the nested name's E, void
                if twin not in fb:
                    print(f"{u} {name}: missing"); rc = 1; continue
                seen.add(twin)
                same = fb[twin] == body
                print(f"{u} {name}: {'same' if same else 'DIFFERENT'} ({len(body)} instructions)")
                rc = rc if same else 1
            for name in sorted(set(fb) - seen):
                print(f"{u} only in B: {name} ({len(fb[name])} instructions)")
    return rc


if __name__ == "__main__":
    sys.exit(main())
