"""The .r1cs reader and the zkey coefficient section it determines (host only, no GPU): every (.r1cs, .zkey) pair the reference ships for
Groth16 pins both exactly — the reader's numbers equal the key's header, and cgh_r1cs_coeff_section is byte-equal to section 4 of the shipped
key.  Each refusal of the reader is exercised on a mutated copy of the multiplier2 file; the edge inputs are test-written files."""
import os
import struct

import pytest

import r1cs_tools as rt
from r1cs_tools import CURVES, PAIRS, fx
from oracle_lib import BN254, BLS12_381
from product import cg, ensure_built


@pytest.mark.parametrize("curve_name,circuit", PAIRS)
def test_info_equals_the_shipped_key_header(curve_name, circuit):
    ensure_built()
    curve = CURVES[curve_name]
    z = cg.host_zkey_info(curve, fx(curve_name, circuit, "circuit.zkey"))
    r = cg.R1cs(curve, fx(curve_name, circuit, "circuit.r1cs"))
    try:
        assert (r.info["n_wires"], r.info["n_public"], r.info["domain_size"], r.info["n_constraints"], r.info["nnz_a"], r.info["nnz_b"]) == \
               (z["n_vars"], z["n_public"], z["domain_size"], z["num_constraints"], z["nnz_a"], z["nnz_b"])
        p = rt.parse_r1cs(fx(curve_name, circuit, "circuit.r1cs"))
        assert (r.info["n_wires"], r.info["n_public"], r.info["n_constraints"]) == (p["n_wires"], p["n_public"], p["n_constraints"])
        assert r.info["nnz_c"] == sum(len(c[2]) for c in p["constraints"])
        assert rt.zkey_header_numbers(curve, rt.zkey_sections(fx(curve_name, circuit, "circuit.zkey"))) == (z["n_vars"], z["n_public"], z["domain_size"])
    finally:
        r.close()


@pytest.mark.parametrize("curve_name,circuit", PAIRS)
def test_coeff_section_is_byte_equal_to_the_shipped_key(curve_name, circuit):
    ensure_built()
    curve = CURVES[curve_name]
    r = cg.R1cs(curve, fx(curve_name, circuit, "circuit.r1cs"))
    try:
        assert r.coeff_section() == rt.zkey_sections(fx(curve_name, circuit, "circuit.zkey"))[4]
    finally:
        r.close()


def test_coeff_section_layout_from_python_integers():
    """the section as the issue describes it, rebuilt record by record from the file with Python integers (value = coef * R^2 mod r)"""
    ensure_built()
    for curve_name, circuit in (("bn254", "kyc"), ("bls12_381", "kyc")):
        curve = CURVES[curve_name]
        p = rt.parse_r1cs(fx(curve_name, circuit, "circuit.r1cs")); mod = rt.modulus(curve)
        recs = []
        for j, con in enumerate(p["constraints"]):
            for m in (0, 1):
                recs += [(m, j, wire, v) for wire, v in con[m]]
        recs += [(0, p["n_constraints"] + s, s, 1) for s in range(p["n_public"] + 1)]
        want = struct.pack("<I", len(recs)) + b"".join(struct.pack("<III", m, j, wire) + (v * rt.R * rt.R % mod).to_bytes(32, "little") for m, j, wire, v in recs)
        r = cg.R1cs(curve, fx(curve_name, circuit, "circuit.r1cs"))
        try:
            assert r.coeff_section() == want
        finally:
            r.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def sections_of(data):
    _, ns = struct.unpack_from("<II", data, 4)
    off, secs = 12, []
    for _ in range(ns):
        i, n = struct.unpack_from("<IQ", data, off); off += 12
        secs.append((i, data[off:off + n])); off += n
    return secs


def mutate(name):
    """a mutated copy of tests/golden/groth16/bn254/multiplier2/circuit.r1cs (1 constraint, 4 wires, 1 public output) as bytes"""
    data = open(fx("bn254", "multiplier2", "circuit.r1cs"), "rb").read()
    secs = sections_of(data)
    assert sorted(i for i, _ in secs) == [1, 2, 3]
    by = dict(secs)
    h, body = bytearray(by[1]), bytearray(by[2])
    order = [i for i, _ in secs]
    build = lambda parts, **kw: rt.file_bytes([(i, bytes(parts[i])) for i in order], **kw)
    parts = {1: h, 2: body, 3: by[3]}
    if name == "magic": return build(parts, magic=b"r1cz")
    if name == "version": return build(parts, version=2)
    if name == "prime":                                  # BLS12-381's r in a file opened as BN254
        h[4:36] = rt.modulus(BLS12_381).to_bytes(32, "little"); return build(parts)
    if name == "field_size":
        parts[1] = rt.header_bytes(rt.modulus(BN254), 4, 1, 0, 2, 4, 1, field_size=48); return build(parts)
    if name == "section_past_eof":                       # the last section claims 8 bytes more than the file holds
        out = bytearray(build(parts)); pos = len(out) - len(parts[order[-1]]) - 8
        out[pos:pos + 8] = struct.pack("<Q", len(parts[order[-1]]) + 8); return bytes(out)
    if name == "truncated": return build(parts)[:-5]
    if name == "missing_header": return rt.file_bytes([(2, bytes(body)), (3, by[3])])
    if name == "missing_constraints": return rt.file_bytes([(1, bytes(h)), (3, by[3])])
    if name == "duplicate_header": return rt.file_bytes([(1, bytes(h)), (1, bytes(h)), (2, bytes(body)), (3, by[3])])
    if name == "duplicate_constraints": return rt.file_bytes([(1, bytes(h)), (2, bytes(body)), (2, bytes(body)), (3, by[3])])
    if name == "term_count":                             # A's term count runs past the section
        body[0:4] = struct.pack("<I", 1000); return build(parts)
    if name == "wire_id":                                # first term of A: wire 4 of 4
        body[4:8] = struct.pack("<I", 4); return build(parts)
    if name == "value":                                  # first value of A = r
        body[8:40] = rt.modulus(BN254).to_bytes(32, "little"); return build(parts)
    if name == "n_public":                               # nPubOut = 4: 4 + 1 > 4 wires
        h[40:44] = struct.pack("<I", 4); return build(parts)
    raise KeyError(name)


REFUSALS = ["magic", "version", "prime", "field_size", "section_past_eof", "truncated", "missing_header", "missing_constraints", "duplicate_header",
            "duplicate_constraints", "term_count", "wire_id", "value", "n_public"]


def open_fds():
    return sorted(os.readlink(os.path.join("/proc/self/fd", f)) for f in os.listdir("/proc/self/fd") if os.path.exists(os.path.join("/proc/self/fd", f)))


@pytest.mark.parametrize("name", REFUSALS)
def test_reader_refuses(name, tmp_path):
    ensure_built()
    cg.load_host()
    path = str(tmp_path / f"{name}.r1cs")
    with open(path, "wb") as f:
        f.write(mutate(name))
    before = open_fds()
    with pytest.raises(cg.BackendError) as e:
        cg.R1cs(BN254, path)
    assert len(str(e.value)) > len("cogroth16_host: "), "a refusal carries a text"
    assert "r1cs" in str(e.value) or "section" in str(e.value)
    assert open_fds() == before, "the refused file is still open"
    os.remove(path)                                       # (and nothing holds it)


def test_unmutated_copy_is_accepted(tmp_path):
    """the mutation helper rebuilds the file from its sections: without a mutation the reader takes it, and gives the fixture's section"""
    ensure_built()
    data = open(fx("bn254", "multiplier2", "circuit.r1cs"), "rb").read()
    path = str(tmp_path / "copy.r1cs")
    with open(path, "wb") as f:
        f.write(rt.file_bytes(sections_of(data)))
    a, b = cg.R1cs(BN254, path), cg.R1cs(BN254, fx("bn254", "multiplier2", "circuit.r1cs"))
    assert a.info == b.info and a.coeff_section() == b.coeff_section()
    a.close(); b.close()


def test_missing_file_and_wrong_curve():
    ensure_built()
    with pytest.raises(cg.BackendError):
        cg.R1cs(BN254, "/nonexistent/circuit.r1cs")
    with pytest.raises(cg.BackendError):
        cg.R1cs(BN254, fx("bls12_381", "multiplier2", "circuit.r1cs"))
    with pytest.raises(cg.BackendError):
        cg.R1cs(7, fx("bn254", "multiplier2", "circuit.r1cs"))


# ---- edge inputs ---------------------------------------------------------------------------------------------------------------------------
def test_sum_arrays_has_no_constraints():
    ensure_built()
    r = cg.R1cs(BN254, fx("bn254", "sum_arrays", "circuit.r1cs"))
    assert (r.info["n_constraints"], r.info["nnz_a"], r.info["nnz_b"], r.info["nnz_c"], r.info["n_public"], r.info["n_wires"], r.info["domain_size"]) == (0, 0, 0, 0, 6, 7, 8)
    sec = r.coeff_section()
    assert struct.unpack_from("<I", sec)[0] == 7 and len(sec) == 4 + 7 * 44          # only the public rows
    r.close()


@pytest.mark.parametrize("curve", [BN254, BLS12_381])
def test_empty_combinations_odd_map_section_and_unknown_section(curve, tmp_path):
    """a test-written file: constraints with an empty A, an empty B, an empty C and all three empty; a section 3 of odd length; an unknown section
    (id 77) in front of the header"""
    ensure_built()
    mod = rt.modulus(curve)
    cons = [([], [(1, 5)], [(2, mod - 1)]),
            ([(3, 7), (0, 1)], [], [(1, 2)]),
            ([(1, 1)], [(2, mod - 1), (3, 9)], []),
            ([], [], []),
            ([(1, 3)], [(1, 4)], [(3, 12)])]
    path = str(tmp_path / "edges.r1cs")
    rt.write_r1cs(path, mod, 4, 1, 1, 1, cons, before=[(77, b"\x01\x02\x03")], map_section=b"\x00" * 13)
    r = cg.R1cs(curve, path)
    assert (r.info["n_wires"], r.info["n_public"], r.info["n_constraints"], r.info["domain_size"]) == (4, 2, 5, 8)
    assert (r.info["nnz_a"], r.info["nnz_b"], r.info["nnz_c"]) == (4, 4, 3)
    recs = []
    for j, con in enumerate(cons):
        for m in (0, 1):
            recs += [(m, j, wire, v) for wire, v in con[m]]
    recs += [(0, 5 + s, s, 1) for s in range(3)]
    want = struct.pack("<I", len(recs)) + b"".join(struct.pack("<III", m, j, wire) + (v * rt.R * rt.R % mod).to_bytes(32, "little") for m, j, wire, v in recs)
    assert r.coeff_section() == want
    r.close()
