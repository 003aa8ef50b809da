"""co-plonk sessions against the file entry (GPU): plain, and one REP3 party over the loopback replay, on synthetic keys
(cgh_synth_plonk_circuit) at 2^16 and 2^20 on BN254 and 2^16 on BLS12-381.  Per case: session open, the proof through the session and
through the file entry (zkey read + upload + p_tau registration and validation each call), the ms per round (file entry run to round k
minus run to round k - 1), and the device memory in use during the proof (hipMemGetInfo sampled every millisecond; peak over the proof,
above what was in use before it).  The kernel-launch count of round 3 comes from a `rocprofv3 --kernel-trace` run of the file entry
(rounds 1-3 minus rounds 1-2; --launches).

    python scripts/plonk_session_timing.py [--cases bn254:16,bn254:20,bls12_381:16] [--reps 3] [--out profiles/plonk_session_timing.txt]
    python scripts/plonk_session_timing.py --launches bn254:16      (one child per count, run under rocprofv3 by the caller)
"""
import argparse
import os
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import importlib                                                                     # noqa: E402
cg = importlib.import_module("collaborative-circom_amd")
import oracle_lib as orc                                                             # noqa: E402

CURVES = {"bn254": cg.BN254, "bls12_381": cg.BLS12_381}


class MemPeak:
    """device memory in use, sampled every millisecond on a thread (torch.cuda.mem_get_info = hipMemGetInfo)"""
    def __init__(self):
        import torch
        self.torch = torch; self.base = self.used(); self.peak = self.base; self.on = True
        self.t = threading.Thread(target=self.run, daemon=True); self.t.start()

    def used(self):
        free, total = self.torch.cuda.mem_get_info(0)
        return total - free

    def run(self):
        while self.on:
            self.peak = max(self.peak, self.used()); time.sleep(0.001)

    def stop(self):
        self.on = False; self.t.join()
        return (self.peak - self.base) / 2 ** 20


def share(curve, vals, rng):
    a = orc.random_field(curve, orc.FR, vals.shape[0], rng); b = orc.random_field(curve, orc.FR, vals.shape[0], rng)
    c = orc.field_op(curve, orc.FR, "sub", orc.field_op(curve, orc.FR, "sub", vals, a), b)
    return [a, b, c], [c, a, b]


def three_parties(run):
    got, errs = [None] * 3, [None] * 3
    def go(i):
        try: got[i] = run(i)
        except Exception as e: errs[i] = e                                             # noqa: BLE001
    th = [threading.Thread(target=go, args=(i,)) for i in range(3)]
    for t in th: t.start()
    for t in th: t.join()
    if any(errs): raise RuntimeError(errs)
    return got


def case(curve_name, log_n, reps, tmp, out):
    curve = CURVES[curve_name]
    zp, wp = os.path.join(tmp, f"{curve_name}_{log_n}.zkey"), os.path.join(tmp, f"{curve_name}_{log_n}.wtns")
    t = time.perf_counter(); cg.host_synth_plonk_circuit(curve, log_n, 1, zp, wp, n_public=2, n_additions=1 << (log_n - 2)); t_gen = time.perf_counter() - t
    w = orc.read_wtns(curve, wp)
    rng = np.random.default_rng(log_n)
    blind = orc.random_field(curve, orc.FR, 11, rng)
    info = cg.host_plonk_zkey_info(curve, zp)
    out(f"\n== {curve_name} 2^{log_n}: {info} (zkey {os.path.getsize(zp) / 2 ** 20:.0f} MiB, generated in {t_gen:.1f} s)")
    t = time.perf_counter(); s = cg.PlonkSession(curve, zp); t_open = time.perf_counter() - t
    out(f"session open: {t_open * 1e3:.1f} ms")
    s.prove_plain(w, blind)                                                            # warm-up
    ts, mem = [], []
    for _ in range(reps):
        m = MemPeak(); _, sec = s.prove_plain(w, blind); mem.append(m.stop()); ts.append(sec)
    out(f"plain, session:    {np.median(ts) * 1e3:9.2f} ms (median of {reps}: {', '.join(f'{x * 1e3:.2f}' for x in ts)}); device memory during the proof: +{max(mem):.0f} MiB")
    cum = []
    for upto in range(1, 6):
        tt = []
        for _ in range(reps):
            t = time.perf_counter(); cg.plonk_prove_plain(curve, zp, w, blind, upto=upto); tt.append(time.perf_counter() - t)
        cum.append(float(np.median(tt)))
    out(f"plain, file entry: {cum[-1] * 1e3:9.2f} ms (median of {reps}, read + upload + p_tau registration + validation included)")
    out("per round (file entry to round k minus to round k-1, ms): " + ", ".join(f"r{k + 1} {(cum[k] - (cum[k - 1] if k else 0)) * 1e3:.2f}" for k in range(5))
        + f"  (r1 includes the file work: {cum[0] * 1e3:.2f})")
    # one REP3 party over the loopback replay: three parties record, then party 0 alone replays its peers' messages
    npub = info["n_public"]
    wa, wb = share(curve, w[npub + 1:], rng)
    hub = cg.LoopbackHub()
    sessions = [s] + [cg.PlonkSession(curve, zp) for _ in range(2)]
    seeds = [bytes([i + 1]) * 32 for i in range(3)]
    rnds = [cg.ChaChaRand(curve, seeds[i], seeds[(i + 2) % 3]) for i in range(3)]
    three_parties(lambda i: sessions[i].prove_rep3_party(w[:npub + 1], wa[i], wb[i], hub.net(i, record=True), rnds[i].table, streams_table=rnds[i].streams))
    for r in rnds: r.close()
    ts, tf, mem = [], [], []
    for _ in range(reps):
        r = cg.ChaChaRand(curve, seeds[0], seeds[2])
        m = MemPeak(); _, sec = s.prove_rep3_party(w[:npub + 1], wa[0], wb[0], hub.replay_net(0), r.table, streams_table=r.streams); mem.append(m.stop()); ts.append(sec)
        r.close()
        r = cg.ChaChaRand(curve, seeds[0], seeds[2])
        t = time.perf_counter(); cg.plonk_prove_rep3_party(curve, zp, w[:npub + 1], wa[0], wb[0], hub.replay_net(0), r.table, upto=5, streams_table=r.streams); tf.append(time.perf_counter() - t)
        r.close()
    out(f"REP3 party 0 (replay), session:    {np.median(ts) * 1e3:9.2f} ms (median of {reps}); device memory during the proof: +{max(mem):.0f} MiB")
    out(f"REP3 party 0 (replay), file entry: {np.median(tf) * 1e3:9.2f} ms (median of {reps})")
    hub.close()
    for x in sessions: x.close()
    os.remove(zp); os.remove(wp)


def launches(spec, upto):
    """one file-entry proof to round `upto` (the caller counts the kernel rows of rocprofv3's trace)"""
    curve_name, log_n = spec.split(":"); curve = CURVES[curve_name]; log_n = int(log_n)
    tmp = tempfile.mkdtemp()
    zp, wp = os.path.join(tmp, "k.zkey"), os.path.join(tmp, "k.wtns")
    cg.host_synth_plonk_circuit(curve, log_n, 1, zp, wp, n_public=2, n_additions=1 << (log_n - 2))
    w = orc.read_wtns(curve, wp)
    cg.plonk_prove_plain(curve, zp, w, orc.random_field(curve, orc.FR, 11, np.random.default_rng(1)), upto=upto)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="bn254:16,bn254:20,bls12_381:16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_session_timing.txt"))
    ap.add_argument("--launches", default=None)
    ap.add_argument("--upto", type=int, default=3)
    a = ap.parse_args()
    if a.launches:
        launches(a.launches, a.upto); return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    def out(s):                                                                       # appended as it comes: a case cut short keeps the ones before
        print(s, flush=True)
        with open(a.out, "a") as f: f.write(s + "\n")
    import torch
    out(f"co-plonk sessions vs file entry on {torch.cuda.get_device_name(0)}; scripts/plonk_session_timing.py --cases {a.cases} --reps {a.reps}")
    with tempfile.TemporaryDirectory() as tmp:
        for spec in a.cases.split(","):
            c, ln = spec.split(":")
            case(c, int(ln), a.reps, tmp, out)


if __name__ == "__main__":
    main()
