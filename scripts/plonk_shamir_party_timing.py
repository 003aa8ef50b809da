"""ONE Shamir party of co-plonk on a session (GPU), against the in-process entry that was the only way to do the same work before:
synthetic keys (cgh_synth_plonk_circuit, n / 4 additions), (n, t) = (3, 1), seeded randomness, full preprocessing
(preprocess = ceil(shamir_pairs / (t + 1))).  Three parties prove once over the recording loopback; party 0 (the king) and party 1 are then
timed ALONE over the replayed traffic (network excluded): `seconds` and `round_seconds[6]` = preprocessing, rounds 1..5 — the median and
the spread of --reps runs after --warmups.  The yardstick is the wall time of the whole cgh_plonk_prove_shamir call on the same key
(three parties side by side on one GPU, the key re-read, lazy batches of 1024).

    python scripts/plonk_shamir_party_timing.py [--cases bn254:14,bn254:16] [--reps 5] [--warmups 2] [--out profiles/plonk_shamir_party_timing.txt]
    python scripts/plonk_shamir_party_timing.py --cases bn254:16 --one-party 1      (the recording proof and ONE replayed party: run it under
                                                                                      `rocprofv3 --kernel-trace --stats` for launch counts)
"""
import argparse
import importlib
import os
import statistics
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
cg = importlib.import_module("collaborative-circom_amd")
import oracle_lib as orc                                                             # noqa: E402

CURVES = {"bn254": cg.BN254, "bls12_381": cg.BLS12_381}
N, T = 3, 1


def parties(run):
    got, errs = [None] * N, [None] * N

    def go(i):
        try: got[i] = run(i)
        except Exception as e: errs[i] = e                                             # noqa: BLE001
    th = [threading.Thread(target=go, args=(i,)) for i in range(N)]
    for t in th: t.start()
    for t in th: t.join()
    if any(errs): raise RuntimeError(errs)
    return got


def spread(xs):
    return f"{statistics.median(xs) * 1e3:9.2f} ms (min {min(xs) * 1e3:.2f}, max {max(xs) * 1e3:.2f}, {len(xs)} runs)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="bn254:14,bn254:16"); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--out", default=None); ap.add_argument("--one-party", type=int, default=None); ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    cg.build()
    lines = [f"co-plonk, ONE Shamir party on a session vs cgh_plonk_prove_shamir; scripts/plonk_shamir_party_timing.py {' '.join(sys.argv[1:])}"]
    say = lambda s: (lines.append(s), print(s, flush=True))
    tmp = tempfile.mkdtemp()
    for case in a.cases.split(","):
        cname, log_n = case.split(":"); log_n = int(log_n); curve = CURVES[cname]; n = 1 << log_n
        zp, wp = os.path.join(tmp, f"{case}.zkey"), os.path.join(tmp, f"{case}.wtns")
        cg.host_synth_plonk_circuit(curve, log_n, 5, zp, wp, n_public=1, n_additions=n // 4)
        w = orc.read_wtns(curve, wp)
        rng = np.random.default_rng(log_n)
        blind = orc.random_field(curve, orc.FR, 11, rng)
        wits = orc.shamir_share(curve, w[2:], N, T, rng); blinds = orc.shamir_share(curve, blind, N, T, rng)
        seeds = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(N)]
        sessions = [cg.PlonkSession(curve, zp) for _ in range(N)]
        pairs = sessions[0].shamir_pairs(T, False); pre = -(-pairs // (T + 1))
        say(f"\n== {cname} 2^{log_n}, (n, t) = ({N}, {T}): shamir_pairs = {pairs}, preprocess = {pre}")
        hub = cg.ShamirLoopbackHub(N)
        t0 = time.perf_counter()
        got = parties(lambda i: sessions[i].prove_shamir_party_seeded(T, w[:2], wits[i], hub.net(i, record=True), seeds[i], blind=blinds[i], preprocess=pre))
        say(f"three parties side by side over the loopback (recording): {(time.perf_counter() - t0) * 1e3:.1f} ms wall; pair_stats of party 0: "
            f"{ {k: v for k, v in got[0][2].items() if k != 'round_seconds'} }")
        assert orc.plonk_verify(curve, zp, got[0][0], w[1:2])
        for party in ([0, 1] if a.one_party is None else [a.one_party]):
            runs = []
            for r in range(1 if a.one_party is not None else a.warmups + a.reps):
                out, sec, st = sessions[party].prove_shamir_party_seeded(T, w[:2], wits[party], hub.replay_net(party), seeds[party], blind=blinds[party], preprocess=pre, timing=True)
                assert all(np.array_equal(out[k], got[0][0][k]) for k in out)
                runs.append((sec, st["round_seconds"]))
            runs = runs[a.warmups:] if a.one_party is None else runs
            say(f"party {party}{' (king)' if party == 0 else ''} alone over the replay, seconds: {spread([x[0] for x in runs])}")
            for j, name in enumerate(("preprocessing", "round 1", "round 2", "round 3", "round 4", "round 5")):
                say(f"    {name:14s} {spread([x[1][j] for x in runs])}")
        hub.close()
        for s in sessions: s.close()
        if a.one_party is None and not a.no_yardstick:
            batches = -(-(pairs + 11) // (1024 * (T + 1)))
            streams = [orc.random_field(curve, orc.FR, batches * 1024 * (1 + 3 * T) + T * pairs + 64, rng) for _ in range(N)]
            ts = []
            for r in range(a.warmups + a.reps):
                t0 = time.perf_counter(); ref = cg.plonk_prove_shamir(curve, zp, N, T, w[:2], wits, blinds, streams, upto=5); ts.append(time.perf_counter() - t0)
            assert all(np.array_equal(ref[0][k], got[0][0][k]) for k in ref[0])
            say(f"yardstick, cgh_plonk_prove_shamir (whole call, 3 parties on one GPU, key re-read, lazy batches): {spread(ts[a.warmups:])}")
    if a.out:
        with open(a.out, "w") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
