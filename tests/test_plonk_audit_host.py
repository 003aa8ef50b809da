"""The yardstick of the Plonk witness check, pinned without a GPU: the gate residual restated with Python integers (plonk_audit_tools.py)
finds no failing row on the six shipped (Plonk .zkey, witness) pairs, and after one witness entry is changed exactly the rows that entry
can reach: the rows whose maps name the wire or an addition fed by it, less the two kinds of row that hold for every witness (the wire's own
public-input gate, and the gates of the additions, whose output the extended witness recomputes from the changed entry)."""
import random

import pytest

import plonk_audit_tools as at
from r1cs_tools import CURVES, NO_ROW


@pytest.mark.parametrize("curve_name,circuit", at.FIXTURES)
def test_shipped_witnesses_satisfy_every_row(curve_name, circuit):
    curve = CURVES[curve_name]
    key = at.Key(curve, at.plonk_fx(curve_name, circuit, "circuit.zkey"))
    _, w = at.read_witness(curve, at.plonk_fx(curve_name, circuit, "witness.wtns"))
    assert key.n in (8, 64) and (circuit != "kyc" or key.n_add == 19)
    assert at.verdict(key.bad_rows(w)) == (0, NO_ROW)
    # the padding rows carry no selector (what makes checking them free for an honest key)
    assert all(q[i] == 0 for q in key.q for i in range(key.nc, key.n))


@pytest.mark.parametrize("curve_name,circuit", at.FIXTURES)
def test_a_changed_entry_breaks_exactly_the_rows_it_reaches(curve_name, circuit):
    curve = CURVES[curve_name]
    key = at.Key(curve, at.plonk_fx(curve_name, circuit, "circuit.zkey"))
    _, w = at.read_witness(curve, at.plonk_fx(curve_name, circuit, "witness.wtns"))
    rnd = random.Random(7)
    fed_an_addition = False
    for wire in range(1, len(w)):                                  # every entry in turn, public and private
        changed = list(w)
        changed[wire] = (w[wire] + rnd.randrange(1, key.r)) % key.r
        rows = key.reached(wire)
        fed_an_addition |= any(wire in (a[0], a[1]) for a in key.adds)
        assert key.bad_rows(changed) == rows, f"wire {wire}"
    assert fed_an_addition == (key.n_add > 0)
