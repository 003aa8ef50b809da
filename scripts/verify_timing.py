"""Timing of Groth16 verification (profiles/verify_timing.txt): the host single-proof check, the GPU batch check per proof at n = 64, 1 024
and 16 384 split into its stages, and the oracle's verifier per proof on one core — the only verifier that existed before, hence the
yardstick.  Every figure is the median of 5 runs after 2 warm-ups.  Proofs are multiplier2 proofs made by the plain prover (1 024 distinct
ones per curve; larger batches repeat them, the coefficients differ per slot).  usage: python scripts/verify_timing.py [--cpu] [out.txt]
(--cpu: the two host figures only, from the shipped proofs; needs no GPU)"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as orc                                    # noqa: E402
from product import cg, ensure_built                        # noqa: E402

STAGES = ("point checks", "Miller kernel + product", "MSM of C", "scalar sums + MSM over IC", "host tail")


def median_of(fn, runs=5, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(runs):
        t = time.perf_counter(); fn(); out.append(time.perf_counter() - t)
    return statistics.median(out)


def main():
    ensure_built()
    cpu_only = "--cpu" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--cpu"]
    lines = ["Groth16 verification, median of 5 runs after 2 warm-ups (scripts/verify_timing.py)"]
    for name, curve in (("bn254", orc.BN254), ("bls12_381", orc.BLS12_381)):
        d = os.path.join(ROOT, "tests", "golden", "groth16", name, "multiplier2")
        vk = cg.VerifyingKey.from_json(curve, os.path.join(d, "verification_key.json"))
        ovk = orc.vk_from_json(curve, os.path.join(d, "verification_key.json"))
        if cpu_only:
            proof = orc.proof_from_json(curve, os.path.join(d, "circom.proof")); pub = orc.public_from_json(curve, os.path.join(d, "public.json"))
            assert vk.verify(proof, pub) and orc.verify(curve, ovk, pub, proof)
            t_host = median_of(lambda: vk.verify(proof, pub)); t_orc = median_of(lambda: orc.verify(curve, ovk, pub, proof))
            lines += [f"{name}", f"  host single proof (cgh_groth16_verify)      {t_host * 1e3:9.3f} ms",
                      f"  oracle verifier per proof, one core          {t_orc * 1e3:9.3f} ms"]
            vk.close()
            continue
        rng = np.random.default_rng(5)
        sess = cg.ProvingSession(curve, os.path.join(d, "circuit.zkey"), precompute=False)
        one = orc.from_dec(curve, orc.FR, 1)
        proofs, pubs = [], []
        for _ in range(1024):
            a, b = orc.random_field(curve, orc.FR, 2, rng); r, s = orc.random_field(curve, orc.FR, 2, rng)
            w = np.stack([one, orc.field_op(curve, orc.FR, "mul", a, b), a, b])
            proofs.append(sess.prove_plain(w, r, s)[0]); pubs.append(w[1:2])
        sess.close()
        proofs, pubs = np.stack(proofs), np.stack(pubs)
        assert vk.verify(proofs[0], pubs[0]) and orc.verify(curve, ovk, pubs[0], proofs[0])
        t_host = median_of(lambda: vk.verify(proofs[0], pubs[0]))
        t_orc = median_of(lambda: orc.verify(curve, ovk, pubs[0], proofs[0]))
        lines += [f"{name}", f"  host single proof (cgh_groth16_verify)      {t_host * 1e3:9.3f} ms",
                  f"  oracle verifier per proof, one core          {t_orc * 1e3:9.3f} ms"]
        for n in (64, 1024, 16384):
            reps = (n + 1023) // 1024
            pf, pb = np.tile(proofs, (reps, 1))[:n], np.tile(pubs, (reps, 1, 1))[:n]
            stages = []

            def run():
                ok, secs = vk.verify_batch(pf, pb, timing=True)
                assert ok
                stages.append(secs)
            total = median_of(run)
            med = [statistics.median(s[i] for s in stages[2:]) for i in range(5)]
            lines.append(f"  batch n = {n:5d}: {total / n * 1e6:9.2f} us per proof ({total * 1e3:8.2f} ms per batch), oracle / batch per proof = {t_orc / (total / n):8.1f}x")
            lines += [f"      {STAGES[i]:28s} {med[i] / n * 1e6:9.2f} us per proof" for i in range(5)]
        vk.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args:
        open(args[0], "a").write(text)


if __name__ == "__main__":
    main()
