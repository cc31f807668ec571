"""The measurements of profiles/qmc_wavefront.md: PathTraceBlockQMC with hpt_set_option("qmc_wavefront") off (megakernel) against on (wavefront form).

  python profiles/qmc_wavefront.py interior      (a) the bench's 1 M-triangle interior, 1920 x 1080, N = W * H generators, 64 spp: off / on alternated
                                                     in one process, one warm-up each, REPS repetitions, min .. max; Mpaths/s, the round count
  python profiles/qmc_wavefront.py small         (c) test_228 and the Cornell box (test_035 under layout 2: its own layout is the sweep, which keeps the
                                                     megakernel) at 1024 x 1024, 64 spp: schedule 0 with the option on (what the rule chooses), and forced
  python profiles/qmc_wavefront.py off           (b) the option-off interior call alone, REPS repetitions: run once per library (HYDRA_HIP_LIB) by
                                                     `python profiles/qmc_wavefront.py ab <other library>`, which alternates this build and the other
  python profiles/qmc_wavefront.py once [on|off] one interior call after a warm-up at 1 spp, for `rocprofv3 --kernel-trace --stats -- python ...`:
                                                     the shade-pass and trace-pass times are the kernels' rows of that run's stats

Times are the launch's event pair (hpt_last_kernel_ms through GetExecutionTime's device-pointer twin, last_kernel_ms); a path is a sample, so
Mpaths/s = S / ms / 1000. The device-pointer entry is used: nothing crosses the bus inside the timed window. Prints one JSON line per table."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPP = int(os.environ.get("QMC_WF_SPP", "64"))
REPS = int(os.environ.get("QMC_WF_REPS", "5"))


def span(v, nd=2):
    return {"min": round(min(v), nd), "max": round(max(v), nd), "all": [round(x, nd) for x in v]}


class Case:
    def __init__(self, scene, layout=0):
        from hydracore3_amd.api import HipIntegrator, _vp
        self.g = g = HipIntegrator(scene, accel_layout=layout)
        self.img = _vp()
        g._chk(g.L.hpt_device_malloc(g.h, g.N * 16, C.byref(self.img)))
        g._chk(g.L.hpt_device_memset(g.h, self.img, 0, g.N * 16))
        self.gens0 = g.random_gens()

    def call(self, on, schedule, spp=SPP):
        """One call from the same generators: (kernel ms, schedule that ran, rounds of a wavefront call). on = None: the option is not touched (a
        library from before it)."""
        g = self.g
        g.set_schedule(schedule)
        if on is not None:
            g.set_option("qmc_wavefront", int(on))
        g.set_random_gens(self.gens0)
        g.path_trace_qmc_block_dev(self.img, spp)
        ms = g.last_kernel_ms()                                              # (waits for the launch's second event)
        ran = g.last_launch()["schedule"]
        return ms, ran, g.last_schedule()[1] if ran == 2 else 0

    def alternate(self, variants):
        """variants: {name: (on, schedule)}; one warm-up each, then REPS rounds over all of them in turn."""
        for on, schedule in variants.values():
            self.call(on, schedule)
        ms = {k: [] for k in variants}
        ran = {}
        for _ in range(REPS):
            for k, (on, schedule) in variants.items():
                t, s, it = self.call(on, schedule)
                ms[k].append(t); ran[k] = (s, it)
        paths = self.g.N * SPP
        return {k: {"ms": span(ms[k]), "mpaths_s": span([paths / t / 1000.0 for t in ms[k]], 1), "schedule": ran[k][0], "rounds": ran[k][1]} for k in variants}


def interior():
    from hydracore3_amd.synth import interior_scene
    return Case(interior_scene(1920, 1080, subdiv=int(os.environ.get("HYDRA_BENCH_SUBDIV", "4"))))


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "interior"
    if mode == "interior":
        c = interior()
        out = c.alternate({"off": (False, 0), "on": (True, 0)})
        out["on_over_off"] = span([a / b for a, b in zip(out["off"]["ms"]["all"], out["on"]["ms"]["all"])], 3)
        print(json.dumps({"a_interior": out, "accel": c.g.accel_info(), "spp": SPP, "reps": REPS}), flush=True)
    elif mode == "small":
        from hydracore3_amd.scene import load_hydra_xml
        for name, layout in (("test_228", 0), ("test_035", 2)):
            sc = load_hydra_xml(os.path.join(ROOT, "tests", "golden", "scenes", name, "statex_00001.xml"), 1024, 1024)
            c = Case(sc, layout)
            out = c.alternate({"rule (schedule 0, option on)": (True, 0), "megakernel (option off)": (False, 0), "forced wavefront (schedule 2, option on)": (True, 2)})
            print(json.dumps({"c_small": name, "layout": c.g.accel_info()["layout"], "tables": out, "spp": SPP}), flush=True)
    elif mode == "off":
        c = interior()
        c.call(None, 0)
        ms = [c.call(None, 0)[0] for _ in range(REPS)]
        print(json.dumps({"lib": os.environ.get("HYDRA_HIP_LIB", "this build"), "off_ms": span(ms), "mpaths_s": span([c.g.N * SPP / t / 1000.0 for t in ms], 1)}), flush=True)
    elif mode == "ab":
        other = os.path.abspath(sys.argv[2])
        for _ in range(int(os.environ.get("QMC_WF_AB_ROUNDS", "2"))):
            for lib in (None, other):
                env = dict(os.environ)
                env.pop("HYDRA_HIP_LIB", None)
                if lib:
                    env["HYDRA_HIP_LIB"] = lib
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "off"], env=env, timeout=600)
    elif mode == "once":
        on = len(sys.argv) < 3 or sys.argv[2] == "on"
        c = interior()
        c.call(on, 0, spp=1)
        t, s, it = c.call(on, 0)
        print(json.dumps({"once": "on" if on else "off", "ms": round(t, 2), "schedule": s, "rounds": it}), flush=True)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
