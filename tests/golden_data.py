"""Loading the golden fixtures (tests/golden/*.npz, written by tests/golden/make_fixtures.py).

A fixture stores its inputs (X, Q, ids) beside the expected outputs. Where the inputs alone
would make the file larger than the repository allows, the fixture stores instead the
arguments of oracle.reference_test_data that produce them (`generator`: n, q, d, seed) and
the SHA-256 of their bytes (`input_sha256`): the inputs are regenerated and must match that
digest bit for bit before a test uses them."""
import hashlib

import numpy as np

import oracle


def input_digest(X, Q, ids):
    h = hashlib.sha256()
    for a in (X, Q, ids):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load_golden(path):
    with np.load(path) as z:
        f = {k: z[k] for k in z.files}
    if "generator" in f:
        n, q, d, seed = (int(x) for x in f["generator"])
        X, Q, ids = oracle.reference_test_data(n, q, d, seed)
        assert input_digest(X, Q, ids) == str(f["input_sha256"]), "regenerated inputs differ from the fixture's"
        f.update(X=X, Q=Q, ids=ids)
    return f
