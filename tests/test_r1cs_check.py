"""The witness check on the GPU (cg_r1cs_check_dev behind cgh_r1cs_check_witness): every expectation is computed with Python integers from
the same .r1cs file.  Kernel forms: 0 = chosen by size (every circuit here has at most 2^13 rows: the wave form), 1 = a lane per row triple,
2 = a wave per row triple; every case runs all three and they must agree."""
import numpy as np
import pytest

import oracle_lib as orc
import r1cs_tools as rt
from r1cs_tools import CURVES, NO_ROW, PAIRS, fx
from oracle_lib import BN254, BLS12_381
from product import cg, ensure_built

pytestmark = pytest.mark.gpu
FORMS = (0, 1, 2)


@pytest.mark.parametrize("curve_name,circuit", PAIRS)
def test_fixture_witnesses(curve_name, circuit):
    ensure_built()
    curve = CURVES[curve_name]; mod = rt.modulus(curve)
    p = rt.parse_r1cs(fx(curve_name, circuit, "circuit.r1cs"))
    w = orc.read_wtns(curve, fx(curve_name, circuit, "witness.wtns"))
    r = cg.R1cs(curve, fx(curve_name, circuit, "circuit.r1cs"))
    try:
        for form in FORMS:
            assert r.check_witness(w, form=form) == (0, NO_ROW)
        ints = rt.from_mont(curve, w)
        for wire, delta in ((len(ints) - 1, 1), (len(ints) // 2, mod - 1), (0, 1)):          # one wire changed (the constant too: a witness is data)
            bad = list(ints); bad[wire] = (bad[wire] + delta) % mod
            want = rt.evaluate(p["constraints"], bad, mod)
            for form in FORMS:
                assert r.check_witness(rt.to_mont(curve, bad), form=form) == want, (wire, form)
        if p["n_constraints"]:
            bad = list(ints); bad[-1] = (bad[-1] + 1) % mod
            assert rt.evaluate(p["constraints"], bad, mod)[0] > 0
    finally:
        r.close()


@pytest.fixture(scope="module", params=[BN254, BLS12_381], ids=["bn254", "bls12_381"])
def skewed(request, tmp_path_factory):
    """the 4 099-row circuit written as .r1cs, and the same rows with `+ 1` (a term on wire 0) in every C: the file no witness row satisfies"""
    ensure_built()
    curve = request.param; mod = rt.modulus(curve)
    n_wires, cons, w = rt.skewed_circuit(curve)
    d = tmp_path_factory.mktemp("skewed")
    path, path_bad = str(d / "skewed.r1cs"), str(d / "all_bad.r1cs")
    rt.write_r1cs(path, mod, n_wires, 0, 0, n_wires - 1, cons)
    cons_bad = [(a, b, c + [(0, 1)]) for a, b, c in cons]
    rt.write_r1cs(path_bad, mod, n_wires, 0, 0, n_wires - 1, cons_bad)
    r, r_bad = cg.R1cs(curve, path), cg.R1cs(curve, path_bad)
    yield dict(curve=curve, mod=mod, n_wires=n_wires, cons=cons, cons_bad=cons_bad, w=w, r=r, r_bad=r_bad)
    r.close(); r_bad.close()


def test_skewed_circuit_shape(skewed):
    info = skewed["r"].info
    assert (info["n_constraints"], info["n_wires"]) == (rt.ROWS, 1 + rt.BASE + rt.ROWS) == (4099, 4300)
    for m in range(3):
        assert {len(c[m]) for c in skewed["cons"]} >= set(rt.LENGTHS)
    assert all((con[1][0][0] == 0) == (i % 3 == 0) for i, con in enumerate(skewed["cons"]) if con[1])
    vals = {v for con in skewed["cons"] for lc in con for _, v in lc}
    assert 1 in vals and skewed["mod"] - 1 in vals and len(vals) > 1000


CASES = {"satisfied": (), "row_0": (0,), "last_row": (rt.ROWS - 1,), "rows_70_and_4000": (70, 4000)}


@pytest.mark.parametrize("case", list(CASES))
def test_skewed_circuit_cases(skewed, case):
    """the rows named are made bad through their output wire (which no other row reads); rows 70 and 4 000 lie in different workgroups of both
    kernel forms (256 rows or 4 rows per workgroup): the minimum crosses workgroups"""
    curve, mod, r = skewed["curve"], skewed["mod"], skewed["r"]
    w = list(skewed["w"])
    for row in CASES[case]:
        w[1 + rt.BASE + row] = (w[1 + rt.BASE + row] + 1) % mod
    want = rt.evaluate(skewed["cons"], w, mod)
    assert want == (len(CASES[case]), min(CASES[case], default=NO_ROW))
    wm = rt.to_mont(curve, w)
    for form in FORMS:
        assert r.check_witness(wm, form=form) == want, form


def test_skewed_circuit_every_row_bad(skewed):
    curve, mod = skewed["curve"], skewed["mod"]
    want = rt.evaluate(skewed["cons_bad"], skewed["w"], mod)
    assert want == (rt.ROWS, 0)
    wm = rt.to_mont(curve, skewed["w"])
    for form in FORMS:
        assert skewed["r_bad"].check_witness(wm, form=form) == want, form
    # and the handle keeps its matrices: the first file's answer is unchanged after the second's calls
    assert skewed["r"].check_witness(wm) == (0, NO_ROW)


def test_device_entry_refuses_bad_arguments():
    ensure_built()
    ctx = cg.Context(0)
    try:
        buf = ctx.alloc(64)
        mats = [(buf, buf, buf)] * 3
        with pytest.raises(cg.BackendError):
            ctx.r1cs_check(BN254, mats, 0, buf, buf, form=3)
        with pytest.raises(cg.BackendError):
            ctx.r1cs_check(BN254, mats, 0, None, buf)
        ctx.r1cs_check(BN254, mats, 0, buf, buf)                       # no rows: count 0, no failing row
        ctx.sync()
        res = buf.download((2,))
        assert (int(res[0]), int(res[1])) == (0, NO_ROW)
        buf.free()
    finally:
        ctx.close()
