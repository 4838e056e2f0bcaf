"""GPU: the output side of the convolutions -- the tile epilogues of csrc/conv_l2.hip with fp32 and with limb-plane output,
conv_l2_fixup_kernel, the activation-stationary kernel's epilogue, and the exact-fp32 conv_epilogue / conv_fixup_kernel -- puts
out the same BITS as at the commit where tests/golden/conv_epilogue_bits.json was recorded (tests/golden/make_conv_epilogue_bits.py:
what is digested, on which kernels and schedules, and why nothing may be unstable here).  A restructuring of those epilogues has
to leave every digest alone; a mismatch after a ROCm or PyTorch update names both toolchains, so that it can be told from a
regression and the fixture recorded again at a known-good commit."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_conv_epilogue_bits as G  # noqa: E402

pytestmark = pytest.mark.gpu


def test_conv_epilogue_outputs_have_the_recorded_bits():
    with open(G.FIXTURE) as f:
        rec = json.load(f)
    assert rec["unstable"] == [], "every sum of these kernels has a fixed order: nothing may be left out"
    now, got = G.toolchain(), G.digests()
    assert sorted(got) == sorted(rec["digests"]), "the generator's outputs changed: record the fixture again at a known-good commit"
    differ = [k for k in sorted(got) if got[k] != rec["digests"][k]]
    print(f"{len(got)} digests compared, {len(differ)} differ")
    assert not differ, (f"{len(differ)} of {len(got)} outputs differ from the recorded bits: {differ[:8]}; recorded with torch "
                        f"{rec['torch']} / HIP {rec['hip']}, now torch {now['torch']} / HIP {now['hip']}")
