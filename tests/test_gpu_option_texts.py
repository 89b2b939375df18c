"""What the three *_set_option entries answer for the option names the handles share, replayed against
tests/golden/option_texts.json: return code and refusal text of every case, exactly as recorded (tools/record_option_texts.py)
from the library before the rules moved into one table (csrc/fic_ctx_options.h)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_option_texts as rec  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "option_texts.json")) as f:
    CASES = json.load(f)["cases"]


def test_the_fixture_holds_the_recorders_cases():
    want = [(h, name, v) for h in rec.HANDLES for name, vals in rec.VALUES.items() for v in vals]
    assert [(c["handle"], c["name"], c["value"]) for c in CASES] == want
    assert any(c["code"] == 0 for c in CASES) and any(c["code"] == -3 for c in CASES)


@pytest.mark.parametrize("handle", list(rec.HANDLES))
def test_codes_and_texts_are_the_recorded_ones(handle):
    cases = [c for c in CASES if c["handle"] == handle]
    got = rec.replay(handle, [(c["name"], c["value"]) for c in cases])
    for c, (code, message) in zip(cases, got):
        assert (code, message) == (c["code"], c["message"]), (handle, c["name"], c["value"])
