"""Generates tests/golden/constructor_s7.json by constructing the REFERENCE ITSELF: the state_dict keys, in order, of
`models.MobileNetSkipAdd((224, 224), pretrained=False)` after torch.manual_seed(7), with the dtype, shape and sha256 of every
tensor.  tests/test_module_surface.py checks the product's constructor against it bit for bit, without the reference at run time.
Test infrastructure; run once, commit the output.  Usage: python -m oracle.make_golden_constructor
"""
import hashlib
import json
import os

import numpy as np
import torch

from oracle.inputs import GOLD

SEED = 7
OUT = os.path.join(GOLD, "constructor_s7.json")


def tensor_record(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return {"dtype": str(a.dtype), "shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def main():
    from oracle.make_golden import import_reference
    ref_models, _ = import_reference()
    torch.manual_seed(SEED)
    sd = ref_models.MobileNetSkipAdd((224, 224), pretrained=False).state_dict()
    with open(OUT, "w") as f:
        json.dump({"seed": SEED, "keys": list(sd), "tensors": {k: tensor_record(v) for k, v in sd.items()}}, f, indent=1)
        f.write("\n")
    print(OUT, len(sd), "tensors")


if __name__ == "__main__":
    main()
