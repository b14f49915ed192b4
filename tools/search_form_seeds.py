#!/usr/bin/env python
"""Seeds of tests/_forms.py (CPU only): for every (case, form) the smallest seed in range(32) under which the oracle's
own runs meet every precondition of tests/_forms.py - the ReLU margin at SEARCH_MARGIN (15; the tests assert 10:
float32 CPU BLAS differs between hosts), every wrong form's beliefs >= 100 x the belief atol away, EuclideanEdge /
LearnedEdge decisions >= 1e-3 from flipping.  Prints the table (ReLU ratio, smallest sensitivity ratio) and the seeds
that are not 0, as the _SEEDS_NOT_0 dict of tests/_forms.py.

    python tools/search_form_seeds.py [case ...]

--sparse: the same for tests/_sparse_forms.py (the SparseGCM cases of tests/test_sparse_forms_*.py; `learned` also
asks for the same selected edges in float32 and float64).

    python tools/search_form_seeds.py --sparse [case ...]
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import _forms as F  # noqa: E402


def main(argv):
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))      # (as tests/conftest.py)
    if "--sparse" in argv:      # the SparseGCM cases: same forms, margins and loop
        import _sparse_forms
        argv = [a for a in argv if a != "--sparse"]
        return search(_sparse_forms, argv, "tests/_sparse_forms.py")
    return search(F, argv, "tests/_forms.py")


def search(F, argv, where):
    cases = argv or list(F.CASES)
    seeds, missing = {}, []
    print("%-9s %-15s %4s %9s %10s %12s %s" % ("case", "form", "seed", "pre-acts", "relu ratio", "sensitivity", "rejected"))
    for case in cases:
        for form in F.forms_of(case):
            rejected = []
            for seed in range(32):
                p = F.preconditions(case, form, seed)
                if not F.failures(p, F.SEARCH_MARGIN):
                    break
                rejected.append(seed)
            else:
                missing.append((case, F.form_id(form)))
                print("%-9s %-15s none in range(32)" % (case, F.form_id(form)))
                sys.stdout.flush()
                continue
            seeds[(case, F.form_id(form))] = seed
            relu = "-" if math.isinf(p.relu_ratio) else "%.1f" % p.relu_ratio
            print("%-9s %-15s %4d %9d %10s %12.0f %s" % (case, F.form_id(form), seed, p.n_pre, relu,
                                                      min(p.sens.values()), rejected))
            sys.stdout.flush()
    print("\n_SEEDS_NOT_0 = {")
    for (case, fid), seed in seeds.items():
        if seed:
            print("    (%r, %r): %d," % (case, fid, seed))
    print("}")
    if missing:
        print("no seed for:", missing, "- shrink B of the case (%s CASES), do not lower the margin" % where)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
