"""Records tests/golden/link_launches.json, the fixture of tests/test_gpu_link_launches.py: the SLUAMD_SOLVE_DEBUG launch lines and solve_launches of that
test's solves, per setting, as the library built in this tree queues them on the device.  Run it at the commit whose launch sequence is to be pinned (the
one before a change to the link drivers of sluamd_factor.cpp), never at the commit under test:
    python tests/golden/make_link_launches.py"""
import json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_link_launches as t

if __name__ == "__main__":
    out = {cfg: t.record(cfg) for cfg in t.CONFIGS}
    with open(os.path.join(HERE, "link_launches.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote link_launches.json:", {cfg: sum(len(v["lines"]) for v in out[cfg].values()) for cfg in out}, "launch lines")
