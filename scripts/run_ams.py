"""A rare-event run on the ocean model, as the reference's run_ams.C: the probability of a
noise-induced transition between two steady states (and with AMS the mean first-passage time).

    python scripts/run_ams.py --preset natl8 --a state_a.h5 --b state_b.h5 [--unstable state_c.h5]
                              [--params params.json] [--set "name=value" ...]

The states are state files (Ocean.saveStateToFile); the model takes its continuation parameters
from state A's file.  The parameters are the reference's names (Transient.hpp:136-172, the theta
stepper's, "sigma", "noise seed", "ams seed", "space", "dof", "snapshot device memory (GB)"), from a
JSON file and / or --set, later ones winning; "dof" defaults to 6 (the ocean score functions).
Prints one JSON line with the estimates.  All of the logic is iemic.rare_event's.
"""
import argparse
import json
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "i-emic_amd"))

from iemic import config as cf                       # noqa: E402
from iemic.ocean import Ocean                        # noqa: E402
from iemic.rare_event import transient_factory       # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", required=True)
    ap.add_argument("--a", required=True)
    ap.add_argument("--b", required=True)
    ap.add_argument("--unstable")
    ap.add_argument("--params")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    logging.basicConfig(level=logging.WARNING if a.quiet else logging.INFO, format="%(message)s")
    params = {"dof": 6}
    if a.params:
        with open(a.params) as f:
            params.update(json.load(f))
    for item in a.set:
        name, _, value = item.partition("=")
        try:
            params[name] = json.loads(value)
        except ValueError:
            params[name] = value
    oc = Ocean(cf.preset(a.preset))
    sols = []
    for path in (a.b, a.unstable, a.a):              # A last: the model keeps its parameters
        if path is None:
            sols.append(None)
            continue
        if oc.loadStateFromFile(path):
            raise SystemExit(f"run_ams: {path} does not exist")
        sols.append(oc.getState().copy())
    tr = transient_factory(oc, params, sols[2], sols[0], sols[1])
    status = tr.run()
    print(json.dumps({"method": tr.method, "status": status, "probability": tr.get_probability(),
                      "mfpt": tr.get_mfpt(), "iterations": tr.its, "time_steps": tr.time_steps,
                      "extinct": tr.extinct, "ams_seed": tr.ams_seed, "noise_seed": tr.stepper.noise_seed}))
    oc.close()


if __name__ == "__main__":
    main()
