"""Timing of Plonk verification (profiles/plonk_verify_timing.txt): (b) the host single-proof check on both curves, (c) the oracle's
plonk_verify per proof on one core — the only Plonk verifier that existed before, hence the reference point — and (d) the GPU batch check
per proof split into its five stages at n = 64, 1 024 and 16 384 on BN254 and at n = 1 024 on BLS12-381.  Every figure is the median of
5 runs after 2 warm-ups.  Batches are tiled from 16 distinct multiplier2 proofs made by the plain prover (the coefficients differ per slot).
(a), the compiler's resource report of the two kernels, comes from a cross-compile of csrc/capi_plonk_verify.hip for gfx950 with
-Rpass-analysis=kernel-resource-usage (--resources: that table only; needs hipcc, no GPU; the compile takes several minutes).
usage: python scripts/plonk_verify_timing.py [--cpu | --resources] [out.txt]     (--cpu: (b) and (c) only, from the shipped proofs; needs no GPU)"""
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as orc                                    # noqa: E402
from product import cg, ensure_built                        # noqa: E402

STAGES = ("point checks", "scalar kernel", "A-side MSM (2n points)", "B-side MSM (9n points)", "host tail")
DISTINCT = 16


def median_of(fn, runs=5, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(runs):
        t = time.perf_counter(); fn(); out.append(time.perf_counter() - t)
    return statistics.median(out)


def resource_report():
    """(a): the compiler's remarks for the kernels of capi_plonk_verify.hip, one table row per kernel"""
    csrc = os.path.join(ROOT, "collaborative-circom_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [os.environ.get("HIPCC", "hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-DCG_WITH_BLS=1",
               "-Wno-unused-result", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "capi_plonk_verify.hip"), "-o", os.path.join(tmp, "unit.o")]
        err = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, check=True).stderr
    fields = ("VGPRs", "AGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            cur = {"name": subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void cg::", "")}
            rows.append(cur)
            continue
        m = re.search(r"remark: +([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in fields:
            cur[m.group(1).strip()] = int(m.group(2))
    out = ["(a) Compiler resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, csrc/capi_plonk_verify.hip), workgroups of 64 lanes",
           f"  {'kernel':66s} VGPRs  AGPRs  SGPRs  VGPR spills  SGPR spills  scratch B/lane  LDS B/workgroup  waves/SIMD"]
    for r in rows:
        out.append(f"  {r['name']:66s} {r.get('VGPRs', 0):5d}  {r.get('AGPRs', 0):5d}  {r.get('TotalSGPRs', 0):5d}  {r.get('VGPRs Spill', 0):11d}  {r.get('SGPRs Spill', 0):11d}  "
                   f"{r.get('ScratchSize [bytes/lane]', 0):14d}  {r.get('LDS Size [bytes/block]', 0):15d}  {r.get('Occupancy [waves/SIMD]', 0):10d}")
    return out


def main():
    if "--resources" in sys.argv:
        text = "\n".join(resource_report()) + "\n"
        print(text)
        args = [a for a in sys.argv[1:] if a != "--resources"]
        if args:
            open(args[0], "a").write(text)
        return
    ensure_built()
    cpu_only = "--cpu" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--cpu"]
    lines = ["Plonk verification, median of 5 runs after 2 warm-ups (scripts/plonk_verify_timing.py)"]
    for name, curve, sizes in (("bn254", orc.BN254, (64, 1024, 16384)), ("bls12_381", orc.BLS12_381, (1024,))):
        d = os.path.join(ROOT, "tests", "golden", "plonk", name, "multiplier2")
        zp = os.path.join(d, "circuit.zkey")
        vk = cg.PlonkVerifyingKey.from_json(curve, os.path.join(d, "verification_key.json"))
        proof = orc.plonk_proof_from_json(curve, os.path.join(d, "circom.proof")); pub = orc.public_from_json(curve, os.path.join(d, "public.json"))
        assert vk.verify(proof, pub) and orc.plonk_verify(curve, zp, proof, pub)
        t_host = median_of(lambda: vk.verify(proof, pub)); t_orc = median_of(lambda: orc.plonk_verify(curve, zp, proof, pub))
        lines += [f"{name}", f"  (b) host single proof (cgh_plonk_verify)         {t_host * 1e3:9.3f} ms",
                  f"  (c) oracle plonk_verify per proof, one core      {t_orc * 1e3:9.3f} ms"]
        if cpu_only:
            vk.close()
            continue
        rng = np.random.default_rng(5)
        sess = cg.PlonkSession(curve, zp, precompute=False)
        npub = sess.info["n_public"]
        one = orc.from_dec(curve, orc.FR, 1)
        dicts, pubs = [], []
        for _ in range(DISTINCT):
            a, b = orc.random_field(curve, orc.FR, 2, rng)
            w = np.stack([one, orc.field_op(curve, orc.FR, "mul", a, b), a, b])
            dicts.append(sess.prove_plain(w, orc.random_field(curve, orc.FR, 11, rng))[0]); pubs.append(w[1:1 + npub])
        sess.close()
        commits = np.stack([np.stack([p[k] for k in orc.PLONK_COMMITS]) for p in dicts]); evals = np.stack([np.stack([p[k] for k in orc.PLONK_EVALS]) for p in dicts])
        pubs = np.stack(pubs)
        assert vk.verify(dicts[0], pubs[0]) and orc.plonk_verify(curve, zp, dicts[0], pubs[0])
        for n in sizes:
            idx = np.arange(n) % DISTINCT
            cm, ev, pb = commits[idx].copy(), evals[idx].copy(), pubs[idx].copy()
            stages = []

            def run():
                ok, secs = vk.verify_batch((cm, ev), pb, timing=True)
                assert ok
                stages.append(secs)
            total = median_of(run)
            med = [statistics.median(s[i] for s in stages[2:]) for i in range(5)]
            lines.append(f"  (d) batch n = {n:5d}: {total / n * 1e6:9.2f} us per proof ({total * 1e3:8.2f} ms per batch), oracle / batch per proof = {t_orc / (total / n):8.1f}x")
            lines += [f"      {STAGES[i]:28s} {med[i] / n * 1e6:9.2f} us per proof" for i in range(5)]
        vk.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args:
        open(args[0], "a").write(text)


if __name__ == "__main__":
    main()
