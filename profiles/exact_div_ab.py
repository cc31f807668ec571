"""A/B of the replayed division (profiles/exact_div.md): a parent library against the built one, alternated on one box, through bench.py.
HYDRA_HIP_LIB selects the library. Stages (any of them, in this order): `headline` three alternated rounds of `bench.py --gpus 1`; `others`
film, dr, spectral and interior --spp 256 --steps 2, three alternated rounds each; `profile` per library a kernel trace with --stats and two SQ
counter passes (--pmc alone), each a run of its own, reduced by profiles/r7_pmc.py. Every run is a child process with its own time limit and the
first bad exit ends the script.
Usage: python profiles/exact_div_ab.py PARENT_LIBRARY.so OUTDIR [stage ...]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT, OUT = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
STAGES = sys.argv[3:] or ["headline", "others", "profile"]
os.makedirs(OUT, exist_ok=True)
LOG = open(os.path.join(OUT, "results.jsonl"), "a")
BENCH = [sys.executable, "bench.py", "--gpus", "1", "--no-build"]
SQ1 = "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_VMEM_RD".split()
SQ2 = "SQ_THREAD_CYCLES_VALU SQ_WAVES SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_WR GRBM_GUI_ACTIVE".split()


def environment(lib):
    env = dict(os.environ)
    env.pop("HYDRA_HIP_LIB", None)
    if lib == "parent":
        env["HYDRA_HIP_LIB"] = PARENT
    return env


def run(tag, lib, extra, limit=200):
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + BENCH + extra, cwd=ROOT, env=environment(lib), capture_output=True, text=True)
    if r.returncode != 0:
        print("FAILED", tag, lib, extra, r.returncode, r.stdout[-2000:], r.stderr[-2000:], flush=True)
        sys.exit(1)
    value = json.loads([l for l in r.stdout.splitlines() if l.startswith("{") and '"value"' in l][-1])["value"]
    rec = {"tag": tag, "lib": lib, "extra": extra, "value": value, "wall_s": round(time.time() - t0, 1)}
    LOG.write(json.dumps(rec) + "\n"); LOG.flush()
    print(json.dumps(rec), flush=True)
    return value


if "headline" in STAGES:
    for _ in range(3):
        for lib in ("parent", "new"):
            run("headline", lib, ["--steps", "3", "--warmup", "1"])
if "others" in STAGES:
    for wl, extra in (("film", []), ("dr", []), ("spectral", []), ("interior", ["--spp", "256", "--steps", "2"])):
        for _ in range(3):
            for lib in ("parent", "new"):
                run(wl, lib, ["--workload", wl] + extra)
if "profile" in STAGES:
    for tag in ("parent", "new"):
        for suffix, opts, steps in (("_stats", ["--kernel-trace", "--stats"], "3"), ("_sq1", ["--pmc"] + SQ1, "1"), ("_sq2", ["--pmc"] + SQ2, "1")):
            with open(os.path.join(OUT, tag + suffix + ".log"), "w") as log:
                r = subprocess.run(["timeout", "-k", "10", "240", "rocprofv3"] + opts + ["--output-format", "csv", "-d", os.path.join(OUT, "prof", tag + suffix), "--"]
                                   + BENCH + ["--steps", steps, "--warmup", "0"], cwd=ROOT, env=environment(tag), stdout=log, stderr=subprocess.STDOUT)
            print("profile", tag, suffix, "rc", r.returncode, flush=True)
            if r.returncode != 0:
                sys.exit(1)
    r = subprocess.run([sys.executable, "profiles/r7_pmc.py", os.path.join(OUT, "prof")], cwd=ROOT, capture_output=True, text=True)
    with open(os.path.join(OUT, "pmc_pair.json"), "w") as f:
        f.write(r.stdout)
    print(r.stdout, r.stderr[-1000:], flush=True)
