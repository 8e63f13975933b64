#!/usr/bin/env python3
"""Drop-and-rest sweep of the compliant-ground plant over the substep h and the stiction speed v_s (profiles/r08/ground.md).

    python tools/ground_sweep.py [--engine host|oracle|energy] [--seconds 1.0] [--substeps 4,8,16] [--vs 0.05,0.1]

The experiment is tests/ground_oracle.py's drop_test: a robot under a joint PD (Mini Cheetah 300 / 6, ANYmal 1800 / 24, recomputed
at every substep) is dropped from 5 mm above the ground and should come to rest.  Reported after `seconds`: max |v| of the end
state and mean(sum f_z) / weight - 1 over the last 0.1 s, for h = 1 ms / substeps.  --engine oracle / energy run the dense numpy
plant (the committed oracle), host the product's math instantiated on the CPU (tools/host_ground.cpp; the same model, ~10x
faster).  No GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import ground_oracle as go
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", default="host", choices=["host", "oracle", "energy"])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--substeps", default="1,2,4,8,16")
    ap.add_argument("--vs", default="0.01,0.05,0.1")
    a = ap.parse_args()
    for model in ("mini_cheetah", "anymal_b"):
        for s in [int(x) for x in a.substeps.split(",")]:
            for vs in [float(x) for x in a.vs.split(",")]:
                r = go.drop_test(model, a.engine, 1e-3 / s, vs, a.seconds)
                print(json.dumps(dict(model=model, engine=a.engine, h=1e-3 / s, v_s=vs, **r)), flush=True)


if __name__ == "__main__":
    main()
