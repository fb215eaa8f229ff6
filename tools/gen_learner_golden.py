"""Record the learner fixture tests/golden/learner_parent_f64.npz.  TEST INFRASTRUCTURE.

Run at the commit BEFORE the learner was rewritten on the rows view ("One policy per agent (DTE)"): the file holds what that
commit's ``gae``, ``sequence_forward``, ``losses`` and ``update`` computed on the chains of tests/learner_golden_util.py (CPU,
float64, ``fused=False``; the module there lists the chains and why the per-agent chain with clipping is not among them).
Run on a later commit, ``--check`` compares within the margin of tests/test_learner_view_host.py and says how many arrays
are no longer bit-identical, which a reordered sum may cause and a wiring error always does, far beyond the margin.  Data only.

    python tools/gen_learner_golden.py            writes the fixture
    python tools/gen_learner_golden.py --check    recomputes and compares every array with the committed file
"""

from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import learner_golden_util as gu  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", gu.FIXTURE + ".npz")


def main() -> int:
    torch.set_num_threads(1)  # (one thread: a reduction's order does not depend on the machine)
    data = gu.run_all()
    print(f"  {gu.FIXTURE}: {len(gu.CHAINS)} chains, {len(data)} arrays, {sum(v.size for v in data.values())} doubles")
    if "--check" not in sys.argv:
        np.savez_compressed(PATH, **data)
        print(f"    {os.path.getsize(PATH) / 1024:.1f} KiB")
        return 0
    bad = inexact = 0
    with np.load(PATH, allow_pickle=False) as z:
        for k in sorted(set(z.files) ^ set(data)):
            print(f"MISMATCH {k}: in one of the two only")
            bad += 1
        for k, v in data.items():
            if k not in z.files:
                continue
            if z[k].shape != v.shape or not (np.abs(z[k] - v) <= gu.MARGIN * np.maximum(1.0, np.abs(z[k]))).all():
                print(f"MISMATCH {k}")
                bad += 1
            elif not np.array_equal(z[k], v):
                inexact += 1
    print(f"    {bad} arrays outside the margin, {inexact} within it but not bit-identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
