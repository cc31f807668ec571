"""A/B of the pass slices' hand-over (profiles/slice_mailbox.md): a parent library against the built one, alternated on one box, through
bench.py. HYDRA_HIP_LIB selects the library, HPT_PASS_SLICE (diagnostic) the passes per work item, since bench.py sets no options. Headline in
three alternated rounds over slices of 32 ... 512 passes, then --emulate-share 2 / 4 / 8, 1024^2 x 512 and x 256 spp, a profile pair at the
headline's best slice (kernel trace with --stats, two SQ counter passes, each a run of its own; reduced by profiles/r7_pmc.py) and 2048^2 x 256 spp.
Every run is a child process with its own time limit and the first bad exit ends the script.
Usage: python profiles/slice_mailbox_ab.py PARENT_LIBRARY.so OUTDIR"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT, OUT = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
os.makedirs(OUT, exist_ok=True)
LOG = open(os.path.join(OUT, "results.jsonl"), "a")
BENCH = [sys.executable, "bench.py", "--gpus", "1", "--no-build"]
SQ1 = "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_VMEM_RD".split()
SQ2 = "SQ_THREAD_CYCLES_VALU SQ_WAVES SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_WR GRBM_GUI_ACTIVE".split()


def environment(lib, slice_):
    env = dict(os.environ)
    env.pop("HPT_PASS_SLICE", None)
    if lib == "parent":
        env["HYDRA_HIP_LIB"] = PARENT
    if slice_ is not None:
        env["HPT_PASS_SLICE"] = str(slice_)
    return env


def run(tag, lib, slice_, extra, limit=150):
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + BENCH + ["--steps", "3", "--warmup", "1"] + extra, cwd=ROOT, env=environment(lib, slice_),
                       capture_output=True, text=True)
    if r.returncode != 0:
        print("FAILED", tag, lib, slice_, extra, r.returncode, r.stdout[-2000:], r.stderr[-2000:], flush=True)
        sys.exit(1)
    value = json.loads([l for l in r.stdout.splitlines() if l.startswith("{") and '"value"' in l][-1])["value"]
    rec = {"tag": tag, "lib": lib, "slice": slice_, "extra": extra, "value": value, "wall_s": round(time.time() - t0, 1)}
    LOG.write(json.dumps(rec) + "\n"); LOG.flush()
    print(json.dumps(rec), flush=True)
    return value


head = {}
for _ in range(3):
    for lib, s in [("parent", None), ("new", 32), ("new", 64), ("new", 128), ("new", 256), ("new", 512)]:
        head.setdefault((lib, s), []).append(run("headline", lib, s, []))
for share in (2, 4, 8):
    for lib, s in [("parent", None), ("new", 0), ("new", 32), ("new", 64), ("new", 128), ("new", 256)]:
        run(f"share{share}", lib, s, ["--emulate-share", str(share)])
for spp, slices in ((512, (0, 32, 64, 128, 256)), (256, (0, 32, 64, 128))):
    run(f"spp{spp}", "parent", None, ["--spp", str(spp)])
    for s in slices:
        run(f"spp{spp}", "new", s, ["--spp", str(spp)])

best = max((k for k in head if k[0] == "new"), key=lambda k: sum(head[k]))[1]
print("best slice on the headline:", best, flush=True)
for tag, lib, s in (("parent", "parent", None), ("new", "new", best)):
    for suffix, opts, steps in (("_stats", ["--kernel-trace", "--stats"], "3"), ("_sq1", ["--kernel-trace", "--pmc"] + SQ1, "1"), ("_sq2", ["--kernel-trace", "--pmc"] + SQ2, "1")):
        with open(os.path.join(OUT, tag + suffix + ".log"), "w") as log:
            r = subprocess.run(["timeout", "-k", "10", "240", "rocprofv3"] + opts + ["--output-format", "csv", "-d", os.path.join(OUT, "prof", tag + suffix), "--"]
                               + BENCH + ["--steps", steps, "--warmup", "0"], cwd=ROOT, env=environment(lib, s), stdout=log, stderr=subprocess.STDOUT)
        print("profile", tag, suffix, "rc", r.returncode, flush=True)
        if r.returncode != 0:
            sys.exit(1)
r = subprocess.run([sys.executable, "profiles/r7_pmc.py", os.path.join(OUT, "prof")], cwd=ROOT, capture_output=True, text=True)
with open(os.path.join(OUT, "pmc_pair.json"), "w") as f:
    f.write(r.stdout)
print(r.stdout, r.stderr[-1000:], flush=True)
for lib, s in [("parent", None), ("new", 0), ("new", 64), ("new", 128)]:
    run("2048x256", lib, s, ["--width", "2048", "--height", "2048", "--spp", "256"])
