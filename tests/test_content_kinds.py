"""What the content kinds of tests/content.py are there for, from the oracle alone (no GPU): tests/test_gpu_content.py
asserts the same shares on the device's records."""
import pytest

from content import CCLM_SHARE, STRIPES_SHARE, cclm_share, content, stripe_modes, stripes_share
from test_gpu_content import CASES


def test_stripe_directions():
    assert [sorted(stripe_modes(d)) for d in (0, 90, 45, 135, 20, 70, 110, 160)] == [
        [50], [18], [2, 66], [34], [58], [10], [26], [42]]


@pytest.mark.parametrize("kind,w,h,qp,depth", [c for c in CASES if c[0] == "cclm" or c[0].startswith("stripes")])
def test_the_oracle_uses_the_tool_a_kind_is_there_for(kind, w, h, qp, depth):
    from oracle import pyoracle as po
    rec = po.encode_picture(*content(kind, w, h, 1234 + w + h + qp), qp, depth)
    if kind == "cclm":
        share, floor = cclm_share(rec), CCLM_SHARE
    else:
        share, floor = stripes_share(float(kind[7:]), rec), STRIPES_SHARE
    print("%s %dx%d qp%d d%d: share %.3f" % (kind, w, h, qp, depth, share))
    assert share >= floor, share
