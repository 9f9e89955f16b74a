"""Generates tests/golden/reference_live_cases.json by EXECUTING the reference's own BruteForceLinearAssignment
(oracle/_ref/librfs_ref.so, built from the unmodified reference sources) on exactly the tables that
tests/test_oracle_combinatorics.py draws for its live comparisons, so that those comparisons also run where the reference
is absent.  Run where the reference is present:  python tests/golden/make_live_reference_fixtures.py
The fixture is data (inputs + reference outputs); no reference source text is stored."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import binding as ob  # noqa: E402
from tests.test_oracle_combinatorics import extended_live_tables, murty_plain_tables  # noqa: E402

ob.build()
ref = ob.load_ref()
assert ref is not None, "oracle/_ref missing: run `make -C oracle ref` with the reference present"
here = os.path.dirname(os.path.abspath(__file__))

plain = []
for Cm in murty_plain_tables():
    want, _ = ob.ref_bruteforce(Cm)
    k = min(200, math.factorial(Cm.shape[0]))
    plain.append(dict(C=Cm.tolist(), scores=want[:k].tolist()))

extended = []
for nR, nC, Cm in extended_live_tables():
    s, _ = ob.ref_bruteforce(Cm, kmax=math.factorial(nR + nC))
    keep = [float(s[i]) for i in range(len(s)) if s[i] >= -1000.0 and (i == 0 or s[i] != s[i - 1])]
    extended.append(dict(nR=nR, nC=nC, C=Cm.tolist(), n_distinct=len(keep), scores=keep[:200]))

with open(os.path.join(here, "reference_live_cases.json"), "w") as fh:
    json.dump(dict(murty_plain=plain, extended=extended), fh, separators=(",", ":"))
print("wrote", len(plain), "plain and", len(extended), "extended cases")
