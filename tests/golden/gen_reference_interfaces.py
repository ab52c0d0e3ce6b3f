#!/usr/bin/env python3
"""Generate tests/golden/reference_interfaces.json: the two interface facts of the reference that the CPU tests check this
build against (build container only, where the reference is mounted).

- "bindings": the ordered parameter names of the reference's pybind functions compute_aabb / raymarch_forward /
  raymarch_backward (extensions/mvpraymarch/mvpraymarch.cpp) and compute_raydirs_forward (extensions/utils/utils.cpp),
  as declared there (tests/test_native_shim.py maps the renamed ones).
- "configs": the `train` keys that ava-256_amd/config.py reads (ddp-train.py:78,82,321,404-430,441), with their values, of
  configs/config.yaml, config-4.yaml and config-256.yaml (tests/test_trainloop.py).

Nothing of the reference's text is stored: names and values only."""
import json
import os
import re

import yaml

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

BINDINGS = [("compute_aabb", "extensions/mvpraymarch/mvpraymarch.cpp"),
            ("raymarch_forward", "extensions/mvpraymarch/mvpraymarch.cpp"),
            ("raymarch_backward", "extensions/mvpraymarch/mvpraymarch.cpp"),
            ("compute_raydirs_forward", "extensions/utils/utils.cpp")]
CONFIGS = ["config.yaml", "config-4.yaml", "config-256.yaml"]
TRAIN_KEYS = ["init_learning_rate", "lr_scheduler_iter", "gamma", "clip", "batchsize", "losses", "nids", "maxiter",
              "num_epochs"]


def cpp_params(path, fn):
    """Ordered parameter names of `fn(...)` as declared in a binding source."""
    src = open(path).read()
    m = re.search(r"\b%s\s*\(([^{;]*?)\)\s*\{" % fn, src, re.S)
    assert m, fn
    names = []
    for part in m.group(1).replace("\n", " ").split(","):
        part = part.split("=")[0].strip()
        if part:
            names.append(part.split()[-1].lstrip("*&"))
    return names


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    out = {"bindings": {fn: {"file": path, "params": cpp_params(os.path.join(REF, path), fn)} for fn, path in BINDINGS},
           "configs": {}}
    for name in CONFIGS:
        with open(os.path.join(REF, "configs", name)) as f:
            train = yaml.safe_load(f)["train"]
        out["configs"][name] = {"train": {k: train[k] for k in TRAIN_KEYS if k in train}}
    with open(os.path.join(HERE, "reference_interfaces.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.join(HERE, "reference_interfaces.json"))
