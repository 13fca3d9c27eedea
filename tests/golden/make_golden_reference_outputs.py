#!/usr/bin/env python3
"""Generate tests/golden/reference_outputs.json by RUNNING THE REFERENCE ITSELF (oracle/_ref, built in place by
oracle/ref_build.sh) on the cases of the tests that compare the oracle with the reference build:

* tests/test_oracle_golden.py -- cov_apply_diag, the operator chain on LIVE x nest, scan_map into float32 / int64 / int32
  maps, pixels_healpix on the boundary pointings, the 24 random chains;
* tests/test_oracle_ground_filter.py -- legendre_templates, bin_proj, bin_invcov, add_templates.

Each array is recorded as its fingerprint (dtype, shape, SHA-256 of its bytes: tests/golden_util.py), the two ground-filter
products that the test compares with a tolerance as their values.  The cases are built by the tests' own functions, so the
file and the tests cannot drift apart.

    python tests/golden/make_golden_reference_outputs.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

import oracle  # noqa: E402
import golden_util as gu  # noqa: E402
import test_oracle_golden as tg  # noqa: E402
import test_oracle_ground_filter as tf  # noqa: E402

ref = oracle.load_ref()
assert ref is not None, "oracle/_ref missing: run oracle/ref_build.sh where the reference sources are present"
TAIL = (False,)


def prints(arrays):
    return {k: gu.fingerprint(v) for k, v in arrays.items()}


out = {"cov_apply_diag": prints(tg.cov_apply_diag_outputs(ref))}     # (no use_accel in this binding)
for name in tg.LIVE:
    for nest in (True, False):
        out["chain/%s/%s" % (name, nest)] = prints(tg.live_chain_outputs(ref, name, nest, TAIL))
for dname, dtype in tg.SCAN_DTYPES.items():
    out["scan_map/%s" % dname] = prints(tg.scan_map_dtype_outputs(ref, dtype, TAIL))
for nside in tg.BOUNDARY_NSIDES:
    out["boundaries/%d" % nside] = prints(tg.pixels_on_boundaries_outputs(ref, nside, TAIL))
for seed in tg.RANDOM_SEEDS:
    out["random/%d" % seed] = prints(tg.random_chain_outputs(ref, seed, TAIL))
gf = tf.reference_kernel_outputs(ref)
out["ground_filter"] = {k: (v.tolist() if k in ("proj", "invcov") else gu.fingerprint(v)) for k, v in gf.items()}

with open(gu.REFERENCE_OUTPUTS, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote %s: %d cases" % (gu.REFERENCE_OUTPUTS, len(out)))
