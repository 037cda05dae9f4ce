"""Record agp_sparse_fit_create / agp_sparse_nll outputs of the two fixed problems of tests/sparse_gradient_cases.py into
tests/golden/sparse_fit_parent.json (or the path given): run on the commit BEFORE a change that must leave them alone."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import albatross_amd as ab  # noqa: E402
from sparse_gradient_cases import golden_model  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sparse_fit_parent.json")
ctx = ab.Context(0)
rec = {}
for which in ("uniform_1d", "ragged_3d"):
    model, ds = golden_model(which, ctx)
    fit = model.fit(ds).get_fit()
    rec[which] = {"fit_nll": fit.nll, "nll": -model.log_likelihood(ds), "information": [float(v) for v in fit.information]}
    print(which, rec[which]["fit_nll"], rec[which]["nll"])
ctx.close()
with open(out, "w") as f:
    json.dump(rec, f, indent=1)
