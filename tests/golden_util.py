"""Load the committed golden vectors (tests/golden/*.npz, produced by the reference itself:
tests/golden/make_golden.py) and check an implementation against them."""
import hashlib
import json
import os

import numpy as np

import cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHAINS = ("chain_a", "chain_b", "chain_c")
#: the reference's own outputs (oracle/_ref) on the cases of the live-reference tests, recorded by
#: tests/golden/make_golden_reference_outputs.py: a fingerprint per array, plain values where a tolerance applies
REFERENCE_OUTPUTS = os.path.join(GOLDEN, "reference_outputs.json")
_reference_outputs = None


def load_chain(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    case = {k[3:]: np.ascontiguousarray(z[k]) for k in z.files if k.startswith("in_")}
    case["intervals"] = case["intervals"].astype(cases.interval_dtype)
    for k in ("n_det", "n_samp", "nside", "rows", "n_pix_submap", "n_submap"):
        case[k] = int(z["meta_" + k])
    want = {k[4:]: z[k] for k in z.files if k.startswith("out_")}
    return case, want, bool(z["meta_nest"]), bool(z["meta_iau"])


def check_chain(impl, name, tail=(), weights_rtol=1e-13, ztol=1e-12):
    case, want, nest, iau = load_chain(name)
    got = cases.run_chain(impl, case, nest=nest, iau=iau, tail=tail)
    assert np.array_equal(got["quats"], want["quats"]), "quats differ from the reference"
    nbad = np.count_nonzero(got["pixels"] != want["pixels"])
    assert nbad == 0, "%d pixel indices differ from the reference" % nbad
    assert np.array_equal(got["hsub"], want["hsub"])
    assert np.array_equal(got["g2l"], want["g2l"])
    np.testing.assert_allclose(got["weights"], want["weights"], rtol=weights_rtol, atol=1e-15)
    zs = np.max(np.abs(want["zmap"]))
    assert np.max(np.abs(got["zmap"] - want["zmap"])) <= ztol * zs
    ts = np.max(np.abs(want["tod"]))
    assert np.max(np.abs(got["tod"] - want["tod"])) <= 10 * ztol * ts
    return got, want


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def fingerprint(a):
    """dtype, shape and SHA-256 of the bytes of an array: equal fingerprints = bit-identical arrays."""
    a = np.ascontiguousarray(a)
    return "%s %s %s" % (a.dtype.str, "x".join(str(n) for n in a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def reference_outputs(key):
    """The recorded outputs of the reference for one case: {name: fingerprint or list of values}."""
    global _reference_outputs
    if _reference_outputs is None:
        with open(REFERENCE_OUTPUTS) as f:
            _reference_outputs = json.load(f)
    return _reference_outputs[key]


def assert_reference_outputs(key, got):
    """Every array of ``got`` is bit for bit the reference's output of the same name for this case."""
    want = reference_outputs(key)
    assert sorted(got) == sorted(want), (key, sorted(got), sorted(want))
    for name, a in got.items():
        assert fingerprint(a) == want[name], (key, name)
