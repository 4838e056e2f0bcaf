"""GPU: the bilinear head kernels of csrc/pointwise.hip put out the same BITS as at the commit where
tests/golden/head_bits.json was recorded (tests/golden/make_head_bits.py: what is digested, and why digests are sound for
kernels with a fixed summation order).  A restructuring of those kernels has to leave every digest alone; a mismatch after a
ROCm or PyTorch update names both toolchains, so that it can be told from a regression and the fixture recorded again at a
known-good commit."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_head_bits as G  # noqa: E402

pytestmark = pytest.mark.gpu


def test_head_outputs_have_the_recorded_bits():
    with open(G.FIXTURE) as f:
        rec = json.load(f)
    now, got = G.toolchain(), G.digests()
    assert sorted(got) == sorted(rec["digests"]), "the generator's outputs changed: record the fixture again at a known-good commit"
    differ = [k for k in sorted(got) if got[k] != rec["digests"][k]]
    print(f"{len(got)} digests, {len(differ)} differ")
    assert not differ, (f"{len(differ)} of {len(got)} outputs differ from the recorded bits: {differ[:8]}; recorded with torch "
                        f"{rec['torch']} / HIP {rec['hip']}, now torch {now['torch']} / HIP {now['hip']}")
