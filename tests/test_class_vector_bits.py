"""GPU: the per-pixel class-vector kernels of csrc/loss_proto.hip -- both loss families, softmax statistics, the prototype
kernels, multi-tensor SGD and EMA -- put out the same BITS as at the commit where tests/golden/class_vector_bits.json was
recorded (tests/golden/make_class_vector_bits.py: what is digested, why digests are sound for kernels with a fixed summation
order, and which keys are left out as unstable).  A restructuring of those kernels has to leave every digest alone; a mismatch
after a ROCm or PyTorch update names both toolchains, so that it can be told from a regression and the fixture recorded again
at a known-good commit."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_class_vector_bits as G  # noqa: E402

pytestmark = pytest.mark.gpu


def test_class_vector_outputs_have_the_recorded_bits():
    with open(G.FIXTURE) as f:
        rec = json.load(f)
    assert all(k.startswith(G.UNSTABLE_PREFIX) for k in rec["unstable"]), "only the monitor means may be left out"
    now, got = G.toolchain(), G.digests()
    assert sorted(got) == sorted(rec["digests"]), "the generator's outputs changed: record the fixture again at a known-good commit"
    compared = [k for k in sorted(got) if k not in rec["unstable"]]
    differ = [k for k in compared if got[k] != rec["digests"][k]]
    print(f"{len(compared)} digests compared ({len(rec['unstable'])} unstable left out), {len(differ)} differ")
    assert not differ, (f"{len(differ)} of {len(compared)} outputs differ from the recorded bits: {differ[:8]}; recorded with torch "
                        f"{rec['torch']} / HIP {rec['hip']}, now torch {now['torch']} / HIP {now['hip']}")
