#!/usr/bin/env python3
"""Times the Plonk development setup from an .r1cs (cgh_setup_plonk_dev: gate compiler, transforms and MSMs on the GPU) beside
cgh_synth_plonk_circuit (random gate lists, one transform per polynomial through host memory, host Horner sums) at the same domain on the
same build, with the setup's own stage times, and the count and emit kernels alone.

The circuit is the chain circuit of r1cs_setup_timing.py (cgh_synth_circuit's, rebuilt as an .r1cs): 2^log - 2 multiplication rows of one
term per combination and one public input, so its Plonk key has 2^log - 1 gates, no additions and the domain 2^log.

    python scripts/plonk_setup_timing.py [--logs 16 20] [--runs 5] [--out profiles/plonk_setup_timing.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from r1cs_setup_timing import ROOT, cg, chain_r1cs, line, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--curve", default="bn254", choices=["bn254", "bls12_381"])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_setup_timing.txt"))
    a = ap.parse_args()
    curve = cg.BN254 if a.curve == "bn254" else cg.BLS12_381
    cg.build()
    lines = [f"plonk_setup_timing.py: {a.curve}, {cg.load().cg_version().decode()}", ""]
    with tempfile.TemporaryDirectory() as d:
        for log_n in a.logs:
            zk, wt, r1, dev, syn, syn_w = (os.path.join(d, n) for n in ("synth.zkey", "synth.wtns", "chain.r1cs", "dev.zkey", "synth_plonk.zkey", "synth_plonk.wtns"))
            cg.host_synth_circuit(curve, log_n, 7, zk, wt, device=a.device)
            n_vars, nc = chain_r1cs(curve, zk, r1)
            w = cg.host_read_wtns(curve, wt)
            r = cg.R1cs(curve, r1)
            assert r.check_witness(w, device=a.device) == (0, cg.NO_ROW)
            info = r.plonk_info(device=a.device)
            assert info == dict(n_additions=0, n_constraints=nc + 1, n_vars=n_vars, domain_size=1 << log_n), info
            print(f"2^{log_n}: circuit ready", flush=True)
            t_synth = timed(lambda: cg.host_synth_plonk_circuit(curve, log_n, 7, syn, syn_w, n_public=1, n_additions=0, device=a.device), a.runs)
            print(f"2^{log_n}: synth timed", flush=True)
            stages = []
            t_setup = timed(lambda: stages.append(cg.setup_plonk(r, 7, dev, device=a.device, timing=True)), a.runs)
            print(f"2^{log_n}: setup timed", flush=True)
            t_info = timed(lambda: r.plonk_info(device=a.device), a.runs)
            sess = cg.PlonkSession(curve, dev, device=a.device)                  # the key is a key: a proof on it verifies
            blind = np.zeros((11, 4), dtype=np.uint64); blind[:, 0] = np.arange(3, 14)
            proof, _ = sess.prove_plain(w, blind)
            assert sess.verify(proof, w[1:2]), "a proof on the development key does not verify"
            sess.close()
            # the kernels alone, operands resident (one term per combination, wires >= 1: the file's CSR is canonical)
            ctx = cg.Context(a.device)
            cons = np.fromfile(r1, dtype=np.dtype([("n", "<u4"), ("wire", "<u4"), ("v", "<u8", 4)]), count=3 * nc, offset=12 + 12 + 64 + 12).reshape(nc, 3)
            row_ptr = np.arange(nc + 1, dtype=np.uint32)
            mats, keep = [], []
            for m in range(3):
                can = np.ascontiguousarray(cons["v"][:, m]); mont = np.empty_like(can)
                assert cg.load().cg_fr_from_canonical(curve, can.ctypes.data_as(C.c_void_p), mont.ctypes.data_as(C.c_void_p), C.c_size_t(nc)) == 0
                bufs = (ctx.to_device(row_ptr), ctx.to_device(np.ascontiguousarray(cons["wire"][:, m])), ctx.to_device(mont))
                mats.append(bufs); keep += bufs
            n = 1 << log_n
            counts, offsets = ctx.alloc((nc + 1) * 4), ctx.alloc((nc + 1) * 4)
            maps, q = [ctx.alloc((nc + 1) * 4) for _ in range(3)], [ctx.alloc(n * 32) for _ in range(5)]
            ids, fs = ctx.alloc(16), ctx.alloc(64)
            t_count = timed(lambda: ctx.plonk_gates_count(curve, mats, nc, 3 * nc, counts, offsets), a.runs)

            def emit():
                ctx.plonk_gates_emit(curve, mats, nc, n_vars, 1, counts, offsets, 0, n, maps, q, ids, fs); ctx.sync()
            t_emit = timed(emit, a.runs)
            ctx.free_many(keep + [counts, offsets, ids, fs] + maps + q); ctx.close(); r.close()
            size = os.path.getsize(dev)
            lines += [f"chain circuit, domain 2^{log_n}: {n_vars} wires, {nc} constraints, 1 public input -> {nc + 1} gates, 0 additions; key file {size / 2**20:.1f} MiB",
                      line("cgh_synth_plonk_circuit (zkey + wtns written)", t_synth),
                      line("cgh_setup_plonk_dev (zkey written)", t_setup)]
            lines += [line(f"    stage: {name}", [s[name] for s in stages[1:]]) for name in cg.PLONK_SETUP_STAGES]
            med = {name: statistics.median(s[name] for s in stages[1:]) for name in cg.PLONK_SETUP_STAGES}
            top = sorted(med, key=med.get, reverse=True)[:2]
            lines.append("      largest stages: " + ", ".join(f"{name} {100 * med[name] / sum(med.values()):.0f} %" for name in top) +
                         " of the stage sum (write = fwrite of the sections; transforms = cg_ntt_dev batches AND the download of their coefficients and evaluations)")
            lines += [line("cgh_r1cs_plonk_info (count pass, resident)", t_info),
                      line("cg_plonk_gates_count_dev alone (count + scan)", t_count),
                      line("cg_plonk_gates_emit_dev alone", t_emit), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
