"""The per-rollout fills' bits, frozen (tests/golden/fill_bits.json, scripts/record_fill_bits.py).

The other tests compare the fill paths with each other (cached = fused, dictionary = full cache,
shards = one launch) and with the oracle to ~1e-11; a sum reordered inside code all the paths
share (csrc/spai_fill.h) would move both sides of each such equality together.  Here every path's
res2, the exact limbs of its last line shard and its M are compared with ``==`` against the bits
recorded before the paths shared that code.  Shapes: B = 11 (a full chunk of 8 + 3, sample groups
4 + 4 + 3, an odd last pair), removal probabilities 0 / 0.2 / 0.5 / 1, n no multiple of 64.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_fill_bits", os.path.join(ROOT, "scripts", "record_fill_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(rec.FIXTURE) as _fh:
    GOLD = json.load(_fh)


def test_fixture_covers_every_case():
    assert sorted(GOLD["cases"]) == sorted(rec.CASES)
    assert (GOLD["B"], GOLD["seed"], GOLD["probs"], GOLD["shard_begin"]) == (rec.B, rec.SEED, list(rec.PROBS),
                                                                             rec.SHARD_BEGIN)
    for case, g in GOLD["cases"].items():
        assert g["n"] % 64 != 0 and g["n"] > rec.SHARD_BEGIN, case


@pytest.mark.parametrize("case", rec.CASES)
def test_fill_bits(case):
    want = GOLD["cases"][case]
    env = rec.make_env(case, GOLD["grids"])
    # the cache form first: a case meant for the dictionary kernels must not run the full-cache ones
    form = rec.cache_form(env)
    fill = case.split("-")[1]
    if fill == "qr":
        assert form == "dict:float64"
    elif fill in ("qr_nodict", "lsq_nodict", "lsq_fp64gram_nodict"):
        assert form.startswith("full:")
    elif fill == "qr_wide":
        assert form == "wide:float64"
    elif fill == "qr_fused":
        assert form == "none"
    assert form == want["cache"]
    got = rec.run_case(case, GOLD["grids"], env)
    assert got["qr_rows"] == want["qr_rows"]
    assert got["n"] == want["n"]
    assert got["res2"] == want["res2"]
    assert got["limbs"] == want["limbs"]
    assert got["m_sha256"] == want["m_sha256"]
