"""CPU, only where the reference binary is built (oracle/_ref/SAGE2): the four commands behind the step-5 goldens (tests/copycount_ref.py) are run again on g6, g7
and g4 and must give the committed files and the committed json, which keeps the fixtures honest."""
import gzip, json, os

import pytest

import copycount_ref as R
import fixtures as fx

pytestmark = pytest.mark.skipif(not os.path.exists(R.REF), reason="the reference binary is not built (oracle/_ref/SAGE2)")


@pytest.mark.parametrize("name", ["g6_k70_150", "g7_palindrome_tandem_k21", "g4_highcopy_k21"])
def test_reference_writes_the_committed_files_again(name, tmp_path):
    inp, outp, g5, log = R.reference_step5(name, str(tmp_path))
    gold = lambda suffix: gzip.open(os.path.join(fx.GOLDEN, name + suffix)).read()
    assert inp == gold(".input.cs2.gz") and outp == gold(".output.cs2.gz") and g5 == gold(".graph5.gz")
    assert R.step5_meta(name, inp, outp, g5, log) == json.load(open(os.path.join(fx.GOLDEN, "step5", name + ".step5.json")))
