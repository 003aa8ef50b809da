#!/usr/bin/env python3
"""Times the general Groth16 development setup (cgh_setup_groth16_dev, from an .r1cs) against cgh_synth_circuit (one hard-wired circuit
shape, field work on the host) on the SAME circuit, and the witness check alone.

For each size the chain circuit of cgh_synth_circuit is made once, its .r1cs is rebuilt from the key's coefficient section (A and B; C is
C[j][j + 2] = 1 by construction) and checked against the witness the generator wrote; then both set-ups run `--runs` times after one
warm-up each.  The witness check is timed through the host entry (witness upload + kernel + result download) and as the kernel alone
(device-resident operands), in both kernel forms.

    python scripts/r1cs_setup_timing.py [--logs 16 20] [--runs 5] [--out profiles/r1cs_setup_timing.txt]
"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cg = importlib.import_module("collaborative-circom_amd")


def zkey_sections(path):
    with open(path, "rb") as f:
        head = f.read(12)
        assert head[:4] == b"zkey"
        out = {}
        for _ in range(struct.unpack_from("<I", head, 8)[0]):
            i, n = struct.unpack("<IQ", f.read(12))
            out[i] = (f.tell(), n); f.seek(n, 1)
    return out


def chain_r1cs(curve, zkey_path, r1cs_path):
    """the .r1cs of the chain circuit, from section 4 of the key cgh_synth_circuit wrote: (n_wires, n_constraints)"""
    secs = zkey_sections(zkey_path)
    fq = 48 if curve == cg.BLS12_381 else 32
    with open(zkey_path, "rb") as f:
        f.seek(secs[2][0] + 4 + fq + 4); prime = f.read(32)
        n_vars, n_pub, domain = struct.unpack("<III", f.read(12))
        f.seek(secs[4][0]); ncoef = struct.unpack("<I", f.read(4))[0]
        rec = np.frombuffer(f.read(ncoef * 44), dtype=np.dtype([("m", "<u4"), ("row", "<u4"), ("wire", "<u4"), ("v", "<u8", 4)]))
    nc = n_vars - 2
    assert n_pub == 1 and ncoef == 2 * nc + 2
    body = rec[:2 * nc]
    assert (body["m"][0::2] == 0).all() and (body["m"][1::2] == 1).all() and (body["row"][0::2] == np.arange(nc)).all()
    vals = np.ascontiguousarray(body["v"])                                   # coef * R^2: two Montgomery reductions give the canonical value
    for _ in range(2):
        out = np.empty_like(vals)
        assert cg.load().cg_fr_to_canonical(curve, vals.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_size_t(vals.shape[0])) == 0
        vals = out
    lc = np.dtype([("n", "<u4"), ("wire", "<u4"), ("v", "<u8", 4)])
    cons = np.zeros((nc, 3), dtype=lc)
    cons["n"] = 1
    cons["wire"][:, 0] = body["wire"][0::2]; cons["v"][:, 0] = vals[0::2]
    cons["wire"][:, 1] = body["wire"][1::2]; cons["v"][:, 1] = vals[1::2]
    cons["wire"][:, 2] = np.arange(nc) + 2; cons["v"][:, 2, 0] = 1
    header = struct.pack("<I", 32) + prime + struct.pack("<IIIIQI", n_vars, 0, 1, n_vars - 2, n_vars, nc)
    labels = np.arange(n_vars, dtype="<u8").tobytes()
    with open(r1cs_path, "wb") as f:
        f.write(b"r1cs" + struct.pack("<II", 1, 3))
        for i, payload in ((1, header), (2, cons.tobytes()), (3, labels)):
            f.write(struct.pack("<IQ", i, len(payload))); f.write(payload)
    return n_vars, nc


def timed(fn, runs):
    fn()                                                                     # warm-up
    out = []
    for _ in range(runs):
        t = time.perf_counter(); fn(); out.append(time.perf_counter() - t)
    return out


def line(name, secs, unit=1e3):
    return f"  {name:<44s} median {statistics.median(secs) * unit:10.3f} ms   min {min(secs) * unit:10.3f}   max {max(secs) * unit:10.3f}   ({len(secs)} runs after one warm-up)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--curve", default="bn254", choices=["bn254", "bls12_381"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_setup_timing.txt"))
    a = ap.parse_args()
    curve = cg.BN254 if a.curve == "bn254" else cg.BLS12_381
    cg.build()
    lines = [f"r1cs_setup_timing.py: {a.curve}, {cg.load().cg_version().decode()}", ""]
    with tempfile.TemporaryDirectory() as d:
        for log_m in a.logs:
            zk, wt, r1, dev = (os.path.join(d, n) for n in ("synth.zkey", "synth.wtns", "chain.r1cs", "dev.zkey"))
            t_synth = timed(lambda: cg.host_synth_circuit(curve, log_m, 7, zk, wt, device=a.device), a.runs)
            n_vars, nc = chain_r1cs(curve, zk, r1)
            w = cg.host_read_wtns(curve, wt)
            r = cg.R1cs(curve, r1)
            assert r.check_witness(w, device=a.device) == (0, cg.NO_ROW), "the generator's witness does not satisfy the rebuilt circuit"
            t_setup = timed(lambda: cg.setup_groth16(r, 7, dev, device=a.device), a.runs)
            with open(zk, "rb") as f1, open(dev, "rb") as f2:               # same circuit: same header numbers and coefficient section
                s1, s2 = zkey_sections(zk), zkey_sections(dev)
                f1.seek(s1[4][0]); f2.seek(s2[4][0])
                assert s1[4][1] == s2[4][1] and f1.read(s1[4][1]) == f2.read(s2[4][1])
            cg.host_set_zkey_validation(False)
            rng = np.random.default_rng(3)
            rs = np.zeros((2, 4), dtype=np.uint64); rs[:, 0] = rng.integers(1, 1 << 62, size=2)
            proof = cg.prove_plain(curve, dev, w, rs[0], rs[1], device=a.device)
            vk = cg.VerifyingKey.from_zkey(curve, dev)
            assert vk.verify(proof, w[1:2]), "a proof on the development key does not verify"
            vk.close()
            cg.host_set_zkey_validation(True)
            t_check = timed(lambda: r.check_witness(w, device=a.device), a.runs)
            # the kernel alone, operands resident
            ctx = cg.Context(a.device)
            info = r.info
            # rebuild the three CSR matrices from the file written above (one term per combination)
            cons = np.fromfile(r1, dtype=np.dtype([("n", "<u4"), ("wire", "<u4"), ("v", "<u8", 4)]), count=3 * nc, offset=12 + 12 + 64 + 12).reshape(nc, 3)
            row_ptr = np.arange(nc + 1, dtype=np.uint32)
            mats, keep = [], []
            for m in range(3):
                can = np.ascontiguousarray(cons["v"][:, m]); mont = np.empty_like(can)
                assert cg.load().cg_fr_from_canonical(curve, can.ctypes.data_as(C.c_void_p), mont.ctypes.data_as(C.c_void_p), C.c_size_t(nc)) == 0
                bufs = (ctx.to_device(row_ptr), ctx.to_device(np.ascontiguousarray(cons["wire"][:, m])), ctx.to_device(mont))
                mats.append(bufs); keep += bufs
            d_w, d_res = ctx.to_device(w), ctx.alloc(16)
            t_kernel = {}
            for form, name in ((1, "lane per row"), (2, "wave per row")):
                def run():
                    ctx.r1cs_check(curve, mats, nc, d_w, d_res, nnz_total=3 * nc, form=form); ctx.sync()
                t_kernel[name] = timed(run, a.runs)
                res = d_res.download((2,))
                assert (int(res[0]), int(res[1])) == (0, cg.NO_ROW)
            ctx.free_many(keep + [d_w, d_res]); ctx.close(); r.close()
            lines += [f"chain circuit, domain 2^{log_m}: {n_vars} wires, {nc} constraints, 1 public input; nnz A, B, C = {info['nnz_a']}, {info['nnz_b']}, {info['nnz_c']}",
                      line("cgh_synth_circuit (zkey + wtns written)", t_synth),
                      line("cgh_setup_groth16_dev (zkey written)", t_setup),
                      line("cgh_r1cs_check_witness (upload + kernel)", t_check)]
            lines += [line(f"cg_r1cs_check_dev alone, {name}", t) for name, t in t_kernel.items()]
            lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
