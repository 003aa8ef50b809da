#!/usr/bin/env python3
"""Times the two questions a Plonk key's user can ask without proving, on development keys of the chain circuit (plonk_setup_timing.py's:
2^log - 2 multiplication rows, one public input, no additions):

  * cgh_plonk_session_check_witness beside cgh_plonk_session_prove_plain + cgh_plonk_session_verify on the same session - before the check
    existed, proving and verifying was the only way to learn whether a witness satisfies a key;
  * where the check's time goes: the witness upload, and cg_plonk_gate_check_dev alone on the 4n selector evaluations as a zkey holds them
    (read with a stride of 4: one 32-byte element per 128 bytes) and on contiguous n-row copies of the selectors (what a session keeps);
  * cgh_plonk_session_audit with its stages.

    python scripts/plonk_audit_timing.py [--logs 16 20] [--runs 5] [--out profiles/plonk_audit_timing.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from r1cs_setup_timing import ROOT, cg, chain_r1cs, line, timed, zkey_sections


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_audit_timing.txt"))
    a = ap.parse_args()
    curve = cg.BN254
    cg.build()
    lines = [f"plonk_audit_timing.py: bn254, {cg.load().cg_version().decode()}", ""]
    with tempfile.TemporaryDirectory() as d:
        for log_n in a.logs:
            zk, wt, r1, dev = (os.path.join(d, f) for f in ("synth.zkey", "synth.wtns", "chain.r1cs", "dev.zkey"))
            cg.host_synth_circuit(curve, log_n, 7, zk, wt, device=a.device)
            n_vars, nc = chain_r1cs(curve, zk, r1)
            w = cg.host_read_wtns(curve, wt)
            r = cg.R1cs(curve, r1)
            cg.setup_plonk(r, 7, dev, device=a.device)
            os.remove(zk)
            n = 1 << log_n
            sess = cg.PlonkSession(curve, dev, device=a.device)
            blind = np.zeros((11, 4), dtype=np.uint64); blind[:, 0] = np.arange(3, 14)

            def prove_and_verify():
                proof, _ = sess.prove_plain(w, blind)
                assert sess.verify(proof, w[1:2])
            t_prove = timed(prove_and_verify, a.runs)
            assert sess.check_witness(w) == (0, cg.NO_ROW)
            t_check = timed(lambda: sess.check_witness(w), a.runs)
            print(f"2^{log_n}: check and proof timed", flush=True)
            audits = []
            t_audit = timed(lambda: audits.append(sess.audit(r1cs=r, seed=bytes(32), timing=True)), a.runs)
            assert all(x[0] == 0 for x in audits), audits[0][:2]
            sess.close(); r.close()
            print(f"2^{log_n}: audit timed", flush=True)
            # the check's parts, operands resident: maps and selectors as the session holds them, read from the key file
            ctx = cg.Context(a.device)
            secs = zkey_sections(dev)
            with open(dev, "rb") as f:
                def body(i, skip=0, count=-1):
                    f.seek(secs[i][0] + skip)
                    return f.read(secs[i][1] - skip if count < 0 else count)
                maps = [ctx.to_device(np.frombuffer(body(4 + k), dtype=np.uint32)) for k in range(3)]
                ev = [np.frombuffer(body(7 + k, skip=n * 32), dtype=np.uint64).reshape(4 * n, 4) for k in range(5)]
            q4 = [ctx.to_device(e) for e in ev]
            q1 = [ctx.to_device(np.ascontiguousarray(e[::4])) for e in ev]
            del ev
            pub, ext, res = ctx.alloc(2 * 32), ctx.alloc((n_vars - 2) * 32), ctx.alloc(16)
            zero_then_pub = np.ascontiguousarray(w[:2]).copy(); zero_then_pub[0] = 0

            def upload():
                pub.upload(zero_then_pub); ext.upload(w[2:]); ctx.sync()
            t_upload = timed(upload, a.runs)

            def kernel(q, stride):
                ctx.plonk_gate_check(curve, maps, nc + 1, q, stride, n, pub, 1, ext, n_vars, res); ctx.sync()
            kernel(q4, 4)
            assert tuple(int(x) for x in res.download((2,))) == (0, cg.NO_ROW)
            t_k4, t_k1 = timed(lambda: kernel(q4, 4), a.runs), timed(lambda: kernel(q1, 1), a.runs)
            ctx.free_many(maps + q4 + q1 + [pub, ext, res]); ctx.close()
            size = os.path.getsize(dev); os.remove(dev)
            med = statistics.median
            lines += [f"chain circuit, domain 2^{log_n}: {n_vars} wires, {nc + 1} gates, 1 public input, 0 additions; key file {size / 2**20:.1f} MiB",
                      line("prove_plain + verify on the session", t_prove),
                      line("check_witness on the session", t_check),
                      f"      the check takes {100 * med(t_check) / med(t_prove):.2f} % of a proof and its verification",
                      line("    part: witness upload (host to device)", t_upload),
                      "    part: additions                             none in the chain circuit (one launch per dependency level otherwise)",
                      line("    part: gate kernel, selectors at stride 4", t_k4),
                      line("    part: gate kernel, contiguous selectors", t_k1),
                      f"      stride 4 minus contiguous: {(med(t_k4) - med(t_k1)) * 1e3:.3f} ms; run-to-run spread (max - min): stride 4 {(max(t_k4) - min(t_k4)) * 1e3:.3f} ms, "
                      f"contiguous {(max(t_k1) - min(t_k1)) * 1e3:.3f} ms; contiguous n-row copies of the five selectors would cost {5 * n * 32 / 2**20:.0f} MiB on the session",
                      line("audit on the session, with the .r1cs", t_audit)]
            lines += [line(f"    stage: {name}", [x[2][name] for x in audits[1:]]) for name in cg.PLONK_AUDIT_STAGES] + [""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
