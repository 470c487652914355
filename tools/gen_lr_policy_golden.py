"""Generate tests/golden/lr_policy.json from the UNMODIFIED reference `slowfast/utils/lr_policy.py` (development machine
only: needs a reference checkout; the tests read the fixture, never the reference).

    python tools/gen_lr_policy_golden.py [--reference /path/to/reference]

The reference module is loaded by path with importlib and RUN; only the numbers it returned are written.  Per parameter
set (the SOLVER keys below) the learning rate of `get_lr_at_epoch` at the listed fractional epochs, as `float.hex()`
strings beside the decimal form: a Python double survives the file bit for bit.
"""
import argparse
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "lr_policy.json")

SETS = {
    # the recipe of configs/ssv2.yaml
    "cosine_warmup": dict(LR_POLICY="cosine", BASE_LR=2e-4, COSINE_END_LR=2e-6, COSINE_AFTER_WARMUP=True,
                          WARMUP_EPOCHS=5.0, WARMUP_START_LR=2e-6, MAX_EPOCH=50, STEPS=[], LRS=[]),
    # an SGD recipe: three drops by 10, no warm-up
    "steps": dict(LR_POLICY="steps_with_relative_lrs", BASE_LR=0.1, COSINE_END_LR=0.0, COSINE_AFTER_WARMUP=False,
                  WARMUP_EPOCHS=0.0, WARMUP_START_LR=0.01, MAX_EPOCH=30, STEPS=[0, 14, 22, 27],
                  LRS=[1, 0.1, 0.01, 0.001]),
    # steps with a warm-up that ends past the first drop: its target is the second plateau's rate
    "steps_warmup": dict(LR_POLICY="steps_with_relative_lrs", BASE_LR=0.03, COSINE_END_LR=0.0,
                         COSINE_AFTER_WARMUP=False, WARMUP_EPOCHS=3.5, WARMUP_START_LR=0.0003, MAX_EPOCH=20,
                         STEPS=[0, 3, 11, 16], LRS=[1, 0.3, 0.09, 0.027]),
}
EPOCHS = {
    "cosine_warmup": [0.0, 0.001, 0.5, 2.25, 4.999, 5.0, 5.001, 7.5, 10.0, 13.37, 20.0, 25.0, 27.5, 33.3, 40.0, 45.0,
                      49.0, 49.5, 49.999, 50.0],
    "steps": [0.0, 0.5, 1.0, 7.25, 13.0, 13.999, 14.0, 14.001, 18.5, 21.999, 22.0, 22.5, 26.0, 26.999, 27.0, 27.001,
              28.5, 29.0, 29.999, 30.0, 31.5],
    "steps_warmup": [0.0, 0.001, 0.5, 1.0, 2.0, 2.999, 3.0, 3.25, 3.499, 3.5, 3.501, 7.0, 10.999, 11.0, 12.5, 15.999,
                     16.0, 18.0, 19.999, 20.0],
}


def load_reference(root):
    path = os.path.join(root, "slowfast", "utils", "lr_policy.py")
    spec = importlib.util.spec_from_file_location("_reference_lr_policy", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SVIT_REFERENCE_ROOT"))
    args = ap.parse_args()
    if not args.reference:
        sys.exit("give --reference (or SVIT_REFERENCE_ROOT): the root of a reference checkout")
    ref = load_reference(args.reference)
    out = {}
    for name, solver in SETS.items():
        cfg = types.SimpleNamespace(SOLVER=types.SimpleNamespace(**solver))
        lrs = [ref.get_lr_at_epoch(cfg, ep)["lr"] for ep in EPOCHS[name]]
        out[name] = {"solver": solver, "epochs": EPOCHS[name], "lr": [float(v) for v in lrs],
                     "lr_hex": [float(v).hex() for v in lrs]}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
