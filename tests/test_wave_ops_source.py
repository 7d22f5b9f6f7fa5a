"""CPU: gms_amd/csrc/hip/wave_ops.hpp is the only file of the library that shuffles by an offset.  Every wave sum, maximum, scan and pair fold
goes through its named trees (down tree: lane 0 holds the result; butterfly: every lane does), so no kernel source spells one out by hand again."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gms_amd", "csrc")
HEADER = os.path.join("hip", "wave_ops.hpp")
SHUFFLES = ("__shfl_down(", "__shfl_xor(", "__shfl_up(")


def _sources():
    for base, _, files in os.walk(CSRC):
        for f in sorted(files):
            if f.endswith((".hip", ".hpp", ".cpp")):
                path = os.path.join(base, f)
                yield os.path.relpath(path, CSRC), open(path, errors="ignore").read()


def test_only_wave_ops_shuffles_by_an_offset():
    texts = dict(_sources())
    assert len(texts) > 20 and HEADER in texts
    users = {call: sorted(name for name, text in texts.items() if call in text) for call in SHUFFLES}
    assert users == {call: [HEADER] for call in SHUFFLES}, users


def test_bk_has_no_wave_sum_of_its_own():
    bk = open(os.path.join(CSRC, "hip", "bk.hip")).read()
    assert not re.search(r"\bwave_sum\w*\s*\([^;{]*\)\s*\{", bk)   # no definition of wave_sum / wave_sum_all …
    assert "wave_sum_all(" in bk and not re.search(r"\bwave_sum\(", bk)   # … and its butterfly sites say which tree they use
