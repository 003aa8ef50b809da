#!/usr/bin/env python3
"""bench.py — Groth16 constraints/sec on MI355X for the co-groth16 hot path (BASELINE.json metric).

N = 1 (the driver's default line).  `value` = what the reference times (co-circom/co-circom/src/bin/co-circom.rs:503-506): ONE REP3 party's
`CoGroth16::prove` (co-groth16/src/groth16.rs:113-326) on a synthetic BN254 R1CS with domain size m = 2^22 (num_constraints = m - 2,
n_public = 1, n_vars = m; nnz(A) = 2/row, nnz(B) = 1/row) through the entry the CLI binds, `cgh_session_prove_rep3_party_ex`: witness shares
in HOST memory in, proof out; the party's 4 x 2^22 ChaCha12 / F::rand masking draws (rep3/rngs.rs:37-46) made inside the call on the GPU, the
two mul_vec exchanges crossing PCIe both ways, the O(1) scalar steps and openings on the host.  The party runs ALONE on the GPU; what its
peers sent in a three-party run on the same session is replayed from page-locked memory (network time excluded) and its
proof must repeat bit for bit.  A "step" of the timed region = one such proof; K of them are bracketed by barrier + synchronize.
(The draw ORDER word stream -> limbs -> rejection is restated from rand_chacha 0.3 / ark-ff 0.4.2: parity unpinned for it)

`step_resident` (same line) = the kernel pipeline alone, the figure rounds 1-3 carried as `value`: all inputs (CSR matrices, witness
shares, masks, the vectors "received" from the previous party, the five zkey-sized base tables) resident in HBM before the timed region:
    2 constraint mat-vecs -> REP3 local product -> 4 x (iNTT, coset shift, NTT) -> REP3 local product
    -> 2 x (iNTT, coset shift, NTT) -> subtraction -> 10 MSMs (h, l, a, b1 in G1 and b2 in G2, x 2 share components).
`sizes` = both figures at the other sizes BASELINE.json's north_star names (2^16, 2^20, 2^24), each with its own roofline triple;
`session.bls12_381` = the second curve of the reference's e2e matrix (tests/tests/circom/e2e_tests/mod.rs:20-106) through the same entry.

N > 1 (one process per GPU, torch.distributed / RCCL; `python bench.py --gpus N` without a launcher starts its own N ranks and refuses a box
with fewer GPUs).  `value` keeps the N = 1 basis: ONE REP3 party through the same entry on a session opened over the job's N GPUs
(cgh_session_open_multi — rank 0's process drives them, as one co-circom process would; the other ranks wait in a host-side barrier).
`step_resident` = STRONG scaling of the resident step over the ranks — the ten MSMs are cut into work units
(whole zkey tables, range-split only as far as balance needs it: full-size launches are the efficient ones) that plan_units()
assigns to ranks; every rank holds only its own table slices, and one all_gather of the unit results (a few KB) + host EC
additions fold the slices (RCCL has no EC-add reduction).  The witness map (NTT stage) runs only where its result is needed:
for N < 4 on the rank that owns the h table; for N >= 4 the six vector pipelines (iNTT, coset shift, NTT of a.a, a.b, b.a, b.b,
c.a, c.b) are spread over the ranks, the h table is range-split over ALL ranks and one all_to_all hands every rank the slices
of the six vectors over its own h range (6 * m/N elements; xGMI is point-to-point, so an evenly split all_to_all uses every
link once), where h = a*b - c and the h-slice MSM are computed.

Prints ONE JSON line (rank 0).  `roofline` = dominant kernel (G1 bucket accumulation) against the HBM peak, measured live
with HIP events on the kernels' own stream; `cpu_baseline` = the oracle's C++ restatement of the same workload on the host.

A plain N = 1 run (`bench.py --gpus 1 --steps K --warmup W`) does only what the headline needs: it opens the session, warms up, times
K proofs through the entry and prints the line.  `--full` adds everything else above: the resident step with its isolated launches,
rooflines and copy ceiling, the entry's extras, `sizes`, the Poseidon fixture, the second curve, the in-run counter passes and
`cpu_baseline`.  `--dump-outputs DIR` writes the last timed proof (or, when the resident step is the headline, its folded MSM results)
as float64 .npy files; the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import importlib
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
cg = importlib.import_module("collaborative-circom_amd")

CURVE = cg.BN254                    # default curve of the line (BASELINE.json metric); --curve bls12_381 runs the same legs on the second curve
MAD_PEAK_T = 30.0                   # sustained v_mad_u64_u32 rate, Tmad/s chip-wide at the 2.3 GHz the chip holds on that loop
                                    # (scripts/microbench_clock.hip, profiles/r02_microbench_clock.txt; a 0.3 ms burst gives 26.4)
HBM_PEAK_GBS = 8000.0               # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable)
# scalar-field constants by curve id: modulus, two-adicity, bits; snarkjs' generator is 5^((r-1) >> s) for both (co-circom-snarks/src/lib.rs:208-221)
FR = {cg.BN254: (21888242871839275222246405745257275088548364400416034343698204186575808495617, 28, 254),
      cg.BLS12_381: (0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001, 32, 255)}
CURVE_NAME = {cg.BN254: "BN254", cg.BLS12_381: "BLS12-381"}
G1_POINT_BYTES = {cg.BN254: 64, cg.BLS12_381: 96}          # packed affine x || y; G2 twice that
MADS_PER_G2_ADD = {cg.BN254: 4538, cg.BLS12_381: 10978}   # Fq2 mixed addition, counted in the gfx950 code (profiles/r05_isa_census_acc_g2.txt, ..._bls12_381.txt)
MADS_PER_G1_ADD = {cg.BN254: 1467, cg.BLS12_381: 3542}     # v_mad_u64_u32 per mixed addition on NL = 9 x 29-bit / 14 x 28-bit lazy limbs: 6 products (2 NL^2) + 2 squarings
                                                           # (NL (NL + 1) / 2 + NL^2) + one fused a*b - c*d (3 NL^2)


def rand_fr(n, device, gen, curve=None):
    """n uniformly random reduced residues of the curve's scalar field as (n, 4) int64 limbs (used as Montgomery representatives)."""
    r, _, bits = FR[CURVE if curve is None else curve]
    top, keep = r >> 192, (1 << (bits - 192)) - 1
    x = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, device=device, generator=gen)
    x[:, 3] &= keep
    bad = x[:, 3] >= top              # equality (p = 2^-62) is treated as a rejection
    while bool(bad.any()):
        k = int(bad.sum())
        y = torch.randint(-2**63, 2**63 - 1, (k, 4), dtype=torch.int64, device=device, generator=gen)
        y[:, 3] &= keep
        x[bad] = y
        bad = x[:, 3] >= top
    return x


class Workload:
    """device-resident inputs of one party-0 prove at domain size m; rank `rank` of `world` owns 1/world of every MSM range"""

    def __init__(self, ctx, log_m, device, rank, world, seed=0xC0C1C0DE, precompute=0, curve=None):
        self.ctx, self.log_m, self.m = ctx, log_m, 1 << log_m
        self.curve = curve = CURVE if curve is None else curve
        m = self.m
        self.nc, self.n_inputs, self.n_aux = m - 2, 2, m - 2
        g = torch.Generator(device=device); g.manual_seed(seed)          # same seed on every rank: identical inputs
        nc, n_aux = self.nc, self.n_aux
        i = torch.arange(nc, device=device, dtype=torch.int64)
        self.rpA = (2 * torch.arange(nc + 1, device=device, dtype=torch.int64)).to(torch.int32)
        colA = torch.stack([2 + i, torch.where(i == 0, torch.ones_like(i), 1 + i)], dim=1).reshape(-1)
        self.colA = colA.to(torch.int32)
        self.rpB = torch.arange(nc + 1, device=device, dtype=torch.int64).to(torch.int32)
        self.colB = (2 + (i * 7 + 3) % n_aux).to(torch.int32)
        self.coA, self.coB = rand_fr(2 * nc, device, g, curve), rand_fr(nc, device, g, curve)
        self.pub = rand_fr(2, device, g, curve)
        self.wa, self.wb = rand_fr(n_aux, device, g, curve), rand_fr(n_aux, device, g, curve)
        self.mask1, self.mask2, self.recv1, self.recv2 = (rand_fr(m, device, g, curve) for _ in range(4))
        z = lambda: torch.zeros((m, 4), dtype=torch.int64, device=device)
        self.aa, self.ab, self.ba, self.bb, self.ca, self.cb, self.ha, self.hb = (z() for _ in range(8))
        self.nnz = int(2 * nc + nc)
        # domain constants (snarkjs roots, co-circom-snarks/src/lib.rs:208-221) computed with Python integers
        r, two_adicity, _ = FR[curve]
        zt = pow(5, (r - 1) >> two_adicity, r)
        root = lambda k: pow(zt, 1 << (two_adicity - k), r)
        mont = lambda v: np.array([((v << 256) % r >> (64 * j)) & (2**64 - 1) for j in range(4)], dtype=np.uint64)
        self.omega, self.coset_g = mont(root(log_m)), mont(root(log_m + 1))
        # MSM work units: whole tables / table slices assigned to ranks, see plan_units()
        self.rank, self.world = rank, world
        self.plan = plan_units(world)
        self.mine = [(t, i, parts) for (t, i, parts, owner) in self.plan if owner == rank]
        t0 = time.time()
        self.tables = {}                                  # (table, i, parts) -> (bases, lo, hi)
        for (t, i, parts) in self.mine:
            n_tab = m if t == "h" else n_aux
            lo, hi = shard_range(n_tab, i, parts)
            self.tables[(t, i, parts)] = (ctx.synth_bases(curve, TABLE_GROUP[t], TABLE_FIRST[t] + lo, hi - lo), lo, hi)
        self.setup_bases_s = time.time() - t0
        # witness-map roles
        self.h_units = [(i, parts, owner) + shard_range(m, i, parts) for (t, i, parts, owner) in self.plan if t == "h"]
        self.owns_h = any(owner == rank for (_, _, owner, _, _) in self.h_units)
        self.distributed = wm_distributed(world)
        self.my_vecs = [v for v in range(WM_VECTORS) if wm_vector_owner(v, world) == rank] if self.distributed else []
        if self.distributed:
            (self.h_lo, self.h_hi), = [(lo, hi) for (_, _, owner, lo, hi) in self.h_units if owner == rank]
            hn = self.h_hi - self.h_lo
            self.hs_a, self.hs_b = (torch.zeros((hn, 4), dtype=torch.int64, device=device) for _ in range(2))
        # zkey registration-time work (untimed, like zkey parsing): per-window precomputed tables, resident across proofs
        t0 = time.time()
        self.precompute = precompute
        if precompute:
            for (bases, lo, hi) in self.tables.values():
                ctx.precompute_bases(bases, precompute if precompute > 0 else 0)      # 0 = library picks by table size
        self.setup_precompute_s = time.time() - t0

    def sl(self, t, rng):
        return t[rng[0]:rng[1]]

    def release(self):
        """give the tables (with their window copies) and the vectors back before the next leg registers its own"""
        for (bases, lo, hi) in self.tables.values():
            bases.release()
        self.tables = {}
        for k in [k for k, v in vars(self).items() if isinstance(v, torch.Tensor)]:
            delattr(self, k)
        torch.cuda.empty_cache()
        torch.cuda.synchronize(); cg.dev_cache_trim(self.ctx.device)      # parked blocks of this leg's sizes: the next leg allocates its own


TABLES = ("h", "l", "a", "b1", "b2")            # zkey queries of create_proof_with_assignment (groth16.rs:248-304)
TABLE_GROUP = {"h": 0, "l": 0, "a": 0, "b1": 0, "b2": 1}
TABLE_FIRST = {"h": 1, "l": 3, "a": 5, "b1": 7, "b2": 1}     # synthetic tables: [(first + i) * G]
# Cost model of the planner (ms on one MI355X; p = points of the unit / 2^20; both share components).  Measured with
# scripts/sweep_precompute.py and the bench stage split (profiles/): a unit has a fixed cost (bucket reduction, launch tail) that
# does not shrink with its size, which is why whole tables are preferred over splitting every MSM N ways.
ACC_COST = {0: [(0.25, 0.85), (0.5, 1.51), (1.0, 2.69), (2.0, 5.06), (4.0, 9.0)],        # group -> [(p, ms)]: accumulate + reduce of a unit,
            1: [(0.25, 2.42), (0.5, 4.37), (1.0, 8.49), (2.0, 14.22), (4.0, 26.16)]}      # excl. the sort schedule; interpolated (scripts/unit_cost_table.py, round 4: bucket sets reduced in batches)
SORT_COST = (0.3, 1.2)                           # digit/sort schedule per (rank, scalar set, range), shared by the tables that use it
WM_COST = 4.0                                    # whole witness map on the rank that owns h (N < 4), after overlap with its aux MSMs
WM_VEC_COST = (0.75, 1.6)                        # distributed witness map: SpMV + products once, then per owned vector pipeline
WM_DISTRIBUTE_MIN_WORLD = 4                      # from this many ranks on: vector pipelines spread over ranks + all_to_all
WM_VECTORS = 6                                   # a.a, a.b, b.a, b.b, c.a, c.b


def wm_distributed(world):
    return world >= WM_DISTRIBUTE_MIN_WORLD      # (tests lower the threshold to push a single rank through the collective path)


def wm_vector_owner(v, world):
    """rank that runs the (iNTT, coset shift, NTT) pipeline of vector v when the witness map is distributed"""
    return v % world


def plan_units(world, log_m=22, with_load=False):
    """Work units of the MSM stage and their owner ranks.
    A unit = (table, i, parts): the MSM of BOTH share components over slice i of `parts` contiguous slices of one table.  Whole
    tables are the preferred unit; a table is range-split only as far as balance needs it.  Every split choice (the three G1
    aux tables alike, the G2 table on its own) is tried, units are assigned longest-processing-time first under the measured
    cost model above, and the plan with the smallest maximum rank load wins (ties: fewer units).  For N >= 4 the h table is
    split over all ranks, slice i on rank i, which is what the witness map's all_to_all delivers.  Deterministic: identical on
    every rank.  Returns [(table, i, parts, owner)]."""
    scale = (1 << log_m) / float(1 << 20)
    dist_wm = wm_distributed(world)

    def sched(u):
        return ("h" if u[0] == "h" else "aux", u[1], u[2])

    def acc_cost(u):
        tab, p = ACC_COST[TABLE_GROUP[u[0]]], scale / u[2]
        if p <= tab[0][0]:
            ms = tab[0][1]
        elif p >= tab[-1][0]:
            ms = tab[-1][1] * p / tab[-1][0]
        else:
            (p0, c0), (p1, c1) = next((lo, hi) for lo, hi in zip(tab, tab[1:]) if lo[0] <= p <= hi[0])
            ms = c0 + (c1 - c0) * (p - p0) / (p1 - p0)
        return ms + (WM_COST * scale / 4.0 if u[0] == "h" and not dist_wm else 0.0)

    def sort_cost(u):
        return SORT_COST[0] + SORT_COST[1] * scale / u[2]

    def assign(splits):
        units = [(t, i, splits[t]) for t in TABLES for i in range(splits[t])]
        load = [0.0] * world; owner = {}; scheds = [set() for _ in range(world)]
        def put(u, r):
            load[r] += acc_cost(u) + (0.0 if sched(u) in scheds[r] else sort_cost(u))
            scheds[r].add(sched(u)); owner[u] = r
        if dist_wm:
            for r in range(world):
                nv = sum(1 for v in range(WM_VECTORS) if wm_vector_owner(v, world) == r)
                load[r] += (WM_VEC_COST[0] + WM_VEC_COST[1] * nv) * scale / 4.0 if nv else 0.0
                put(("h", r, world), r)
        rest = [u for u in units if u not in owner]
        for u in sorted(rest, key=lambda u: (-acc_cost(u), u)):
            put(u, min(range(world), key=lambda r: (load[r] + acc_cost(u) + (0.0 if sched(u) in scheds[r] else sort_cost(u)), r)))
        return load, owner, units

    best = None
    g1_choices = [c for c in (1, 2, 3, 4, 6, 8) if c <= max(1, world)]
    g2_choices = [c for c in range(1, 2 * world + 1)]
    for s1 in g1_choices:
        for s2 in g2_choices:
            splits = {"h": world if dist_wm else 1, "l": s1, "a": s1, "b1": s1, "b2": s2}
            load, owner, units = assign(splits)
            key = (round(max(load), 6), len(units))
            if best is None or key < best[0]:
                best = (key, splits, owner, load)
    _, sp, owner, load = best
    plan = [(t, i, sp[t], owner[(t, i, sp[t])]) for t in TABLES for i in range(sp[t])]
    return (plan, load) if with_load else plan


def shard_range(n, rank, world):
    """contiguous range of rank `rank` when n items are split over `world` ranks (sizes differ by at most one)"""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def combine_partials(curve, group, partials):
    """sum of the per-rank partial MSM results (Jacobian) — the 'reduce' of the all_gather + add scheme"""
    acc = partials[0]
    for p in partials[1:]:
        acc = cg.point_add(curve, group, acc, p)
    return acc


def witness_map_local(w):
    """whole witness map on this rank (groth16.rs:143-231): h = FFT_coset(a) * FFT_coset(b) - FFT_coset(c)"""
    ctx, m, nc, C = w.ctx, w.m, w.nc, w.curve
    # constraint evaluation (groth16.rs:159-171), party 0
    ctx.spmv_csr(C, w.rpA, w.colA, w.coA, nc, w.pub, w.n_inputs, 0, w.wa, w.wb, w.aa, w.ab)
    ctx.spmv_csr(C, w.rpB, w.colB, w.coB, nc, w.pub, w.n_inputs, 0, w.wa, w.wb, w.ba, w.bb)
    w.aa[nc:nc + 2] = w.pub                                       # promote_to_trivial_shares + clone_from_slice (party 0 -> component a)
    for v in (w.ab, w.ba, w.bb):
        v[nc:] = 0                                                # rows past the constraints are zero (the buffers are reused in place)
    # c = mul_vec(a, b): local part on the GPU, the other component arrives from the previous party (resident stand-in)
    ctx.vec_rep3_mul_local(C, w.ca, w.aa, w.ab, w.ba, w.bb, w.mask1, m)
    w.cb.copy_(w.recv1)
    vec4 = [w.aa, w.ab, w.ba, w.bb]
    ctx.ntt_coset_pair_dev(C, vec4, m, w.omega, w.coset_g)                  # ifft + distribute_powers + fft in one call
    ctx.vec_rep3_mul_local(C, w.ha, w.aa, w.ab, w.ba, w.bb, w.mask2, m)
    w.hb.copy_(w.recv2)
    ctx.ntt_coset_pair_dev(C, [w.ca, w.cb], m, w.omega, w.coset_g)
    ctx.vec_sub(C, w.ha, w.ha, w.ca, m)
    ctx.vec_sub(C, w.hb, w.hb, w.cb, m)


def a2a_splits(world, rank, h_units, m):
    """all_to_all row counts of the distributed witness map: rank s sends to rank r the slices [lo_r, hi_r) of the vectors s owns.
    Returns (rows this rank sends to each rank, rows it receives from each rank)."""
    rng = {owner: (lo, hi) for (_, _, owner, lo, hi) in h_units}
    nv = lambda r: sum(1 for v in range(WM_VECTORS) if wm_vector_owner(v, world) == r)
    send = [nv(rank) * (rng[r][1] - rng[r][0]) for r in range(world)]
    recv = [nv(s) * (rng[rank][1] - rng[rank][0]) for s in range(world)]
    return send, recv


def wm_exchange(comm, vecs, my_vecs, h_units, world, rank, m):
    """the all_to_all of the distributed witness map: `vecs[v]` (rows x 4 limbs) is valid on the rank that owns v; returns
    {v: rows [lo, hi) of vector v} for this rank's h range, for all six vectors"""
    send_rows, recv_rows = a2a_splits(world, rank, h_units, m)
    rng = {owner: (lo, hi) for (_, _, owner, lo, hi) in h_units}
    like = vecs[0]
    pieces = [vecs[v][rng[r][0]:rng[r][1]] for r in range(world) for v in my_vecs]
    send = torch.cat(pieces) if pieces else torch.empty((0, like.shape[1]), dtype=like.dtype, device=like.device)
    recv = torch.empty((sum(recv_rows), like.shape[1]), dtype=like.dtype, device=like.device)
    comm.all_to_all_rows(recv, send, recv_rows, send_rows)
    hn = rng[rank][1] - rng[rank][0]
    sl, off = {}, 0
    for s_rank in range(world):
        for v in range(WM_VECTORS):
            if wm_vector_owner(v, world) == s_rank:
                sl[v] = recv[off:off + hn]; off += hn
    return sl


def witness_map_distributed(w):
    """world >= 4: this rank runs the pipelines of the vectors it owns, then one all_to_all hands every rank the slices of all six
    coset-evaluation vectors over its own h range, where h = a*b - c is formed (same arithmetic as witness_map_local)."""
    ctx, m, nc, C, world, rank = w.ctx, w.m, w.nc, w.curve, w.world, w.rank
    vecs = [w.aa, w.ab, w.ba, w.bb, w.ca, w.cb]
    if w.my_vecs:
        ctx.spmv_csr(C, w.rpA, w.colA, w.coA, nc, w.pub, w.n_inputs, 0, w.wa, w.wb, w.aa, w.ab)
        ctx.spmv_csr(C, w.rpB, w.colB, w.coB, nc, w.pub, w.n_inputs, 0, w.wa, w.wb, w.ba, w.bb)
        w.aa[nc:nc + 2] = w.pub
        for v in (w.ab, w.ba, w.bb):
            v[nc:] = 0
        if 4 in w.my_vecs:
            ctx.vec_rep3_mul_local(C, w.ca, w.aa, w.ab, w.ba, w.bb, w.mask1, m)
        if 5 in w.my_vecs:
            w.cb.copy_(w.recv1)
        mine = [vecs[v] for v in w.my_vecs]
        ctx.ntt_coset_pair_dev(C, mine, m, w.omega, w.coset_g)
    hn = w.h_hi - w.h_lo
    if w.emulate:       # planner tuning on one GPU: no peers; time the local work only
        sl = {v: vecs[v][w.h_lo:w.h_hi] for v in range(WM_VECTORS)}
    else:
        sl = wm_exchange(w.comm, vecs, w.my_vecs, w.h_units, world, rank, m)
    ctx.vec_rep3_mul_local(C, w.hs_a, sl[0], sl[1], sl[2], sl[3], w.mask2[w.h_lo:w.h_hi], hn)
    w.hs_b.copy_(w.recv2[w.h_lo:w.h_hi])
    ctx.vec_sub(C, w.hs_a, w.hs_a, sl[4], hn)
    ctx.vec_sub(C, w.hs_b, w.hs_b, sl[5], hn)


class Comm:
    """torch.distributed plumbing.  nccl (= RCCL): device tensors straight through.  gloo (tests: several ranks sharing one GPU):
    staged through host memory."""

    def __init__(self, dist, world, device):
        self.dist, self.world, self.device = dist, world, device
        self.host = dist is not None and dist.get_backend() == "gloo"

    def all_to_all_rows(self, recv, send, recv_rows, send_rows):
        if self.dist is None:
            recv.copy_(send); return
        if self.host:
            r = torch.empty(recv.shape, dtype=recv.dtype)
            self.dist.all_to_all_single(r, send.cpu(), recv_rows, send_rows)
            recv.copy_(r)
        else:
            self.dist.all_to_all_single(recv, send, recv_rows, send_rows)

    def all_gather_flat(self, flat_np):
        if self.dist is None:
            return [flat_np]
        t = torch.from_numpy(flat_np.view(np.int64))
        if not self.host:
            t = t.to(self.device)
        out = [torch.empty_like(t) for _ in range(self.world)]
        self.dist.all_gather(out, t)
        return [o.cpu().numpy().view(np.uint64) for o in out]

    def max_float(self, x):
        if self.dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=None if self.host else self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())


def step(w):
    """one pass of the hot path; returns the 10 (partial) MSM results of this rank"""
    ctx, m, nc = w.ctx, w.m, w.nc
    C = w.curve
    # MSM work units of this rank (groth16.rs:248-304).  Units that multiply the same scalar slice share one digit/sort schedule
    # (l, a, b1, b2 all take the aux-witness shares).
    groups = {}
    for key in w.mine:
        t, i, parts = key
        bases, lo, hi = w.tables[key]
        groups.setdefault(("h" if t == "h" else "aux", lo, hi), []).append((key, bases))
    pending = []
    if w.pcie is not None:                       # host -> device: the witness shares first (the aux MSMs start on them) ...
        for dev_t, host_t in w.pcie["up"][:2]:
            dev_t.copy_(host_t, non_blocking=True)
        torch.cuda.current_stream().synchronize()   # the second context must not start on stale shares

    def begin(on, kinds):
        for (kind, lo, hi), members in groups.items():
            if kind not in kinds:
                continue
            members.sort(key=lambda kb: TABLE_GROUP[kb[0][0]] if w.g2_last else -TABLE_GROUP[kb[0][0]])
            if kind == "h":
                sc = [w.hs_a, w.hs_b] if w.distributed else [w.ha[lo:hi], w.hb[lo:hi]]
            else:
                sc = [w.wa[lo:hi], w.wb[lo:hi]]
            tk = on.msm_dev_begin_multi([b for _, b in members], sc, hi - lo)
            pending.extend((on, key, t) for (key, _), t in zip(members, tk))

    # The aux-witness MSMs do not depend on the witness map: they are enqueued first, on a second context (own streams), so that
    # the HBM/LDS-bound witness map runs underneath their integer-VALU-bound bucket accumulation.
    if w.ctx_aux is not None:
        begin(w.ctx_aux, ("aux",))
    if w.pcie is not None:                       # ... then masks and the vectors received from the previous party, in stream order
        for dev_t, host_t in w.pcie["up"][2:]:
            dev_t.copy_(host_t, non_blocking=True)
    if w.distributed:
        witness_map_distributed(w)
    elif w.owns_h:
        witness_map_local(w)
    if w.pcie is not None and not w.distributed and w.owns_h:   # device -> host: the local products sent to the next party
        for dev_t, host_t in w.pcie["down"]:
            host_t.copy_(dev_t, non_blocking=True)
    begin(ctx, ("h",) if w.ctx_aux is not None else ("h", "aux"))
    return {key: on.msm_end(t) for on, key, t in pending}


def unit_layout(plan, curve=None):
    """flat layout of all unit results (2 components x Jacobian) in plan order: {unit: (offset_words, words_per_component)}"""
    off, lay = 0, {}
    nq = 6 if (CURVE if curve is None else curve) == cg.BLS12_381 else 4          # 64-bit words per base-field element
    for (t, i, parts, owner) in plan:
        wlen = 3 * nq if TABLE_GROUP[t] == 0 else 6 * nq
        lay[(t, i, parts)] = (off, wlen, owner)
        off += 2 * wlen
    return lay, off


def exchange(results, plan, comm, curve=None):
    """Each rank contributes the results of its own units (zeros elsewhere); one all_gather of the flat buffer (a few KB), then
    per table the slices are folded with host EC additions (RCCL has no EC-add reduction).  Returns {table: (2, words)}."""
    lay, total = unit_layout(plan, curve)
    flat = np.zeros(total, dtype=np.uint64)
    for key, r in results.items():
        off, wlen, _ = lay[key]
        flat[off:off + 2 * wlen] = r.reshape(-1)
    per_rank = comm.all_gather_flat(flat)
    final = {}
    for (t, i, parts, owner) in plan:
        off, wlen, _ = lay[(t, i, parts)]
        piece = per_rank[owner][off:off + 2 * wlen].reshape(2, wlen)
        if t not in final:
            final[t] = piece.copy()
        else:
            group = cg.G1 if TABLE_GROUP[t] == 0 else cg.G2
            final[t] = np.stack([combine_partials(CURVE if curve is None else curve, group, [final[t][j], piece[j]]) for j in range(2)])
    return final


COMPACT_LIMIT = 8192             # bytes: the driver's parser lost the 21.9 KB line of round 5 (BENCH_r05.json: parsed = null)


def _r(x, nd=4):
    """round floats for the compact line (significant digits, not decimals)"""
    if isinstance(x, float):
        return float(f"{x:.{nd + 3}g}")
    return x


def compact_line(out, detail_path):
    """The ONE line the driver parses: the contract's keys + `roofline` + `cpu_baseline` + the headline figures of every leg, <= COMPACT_LIMIT
    bytes.  Everything else (notes, per-leg rooflines, stage tables, zkey setup times ...) is the full object, written to `detail_path`."""
    pick = lambda d, keys: {k: _r(d[k]) for k in keys if isinstance(d, dict) and k in d and d[k] is not None}
    cfg = out.get("config", {})
    line = {k: _r(out.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline")}
    line["dtype"] = "u32"                                 # 32-bit limbs of 254 / 255 / 381-bit modular integers (v_mad_u64_u32); no floating point anywhere
    line["data"] = out.get("data", "synthetic")
    line["config"] = pick(cfg, ("workload", "num_constraints", "domain_size", "nnz", "share_components", "msm", "ntt"))
    basis = out.get("value_basis", "")
    line["value_basis"] = basis.split(":")[0].split(" — ")[0][:160]
    line["rccl_ranks_seen"] = out.get("rccl_ranks_seen")
    rf = out.get("roofline") or {}
    if rf:                                                # (a plain N = 1 run has the headline only: rooflines come with --full)
        line["roofline"] = pick(rf, ("bound", "achieved", "peak", "unit", "frac", "traffic", "launch_ms", "algorithmic_bytes_per_launch", "measured_copy_ceiling_GBs"))
        line["roofline"]["traffic"] = rf.get("traffic")   # null stays on the line
        line["roofline"]["kernel"] = (rf.get("kernel") or "").split(" (")[0]
    vr = out.get("valu_roofline") or {}
    if vr:
        line["valu_roofline"] = pick(vr, ("achieved", "peak", "frac", "unit"))
    for name in ("roofline_g2", "roofline_ntt"):
        if out.get(name):
            line[name] = pick(out[name], ("achieved", "frac", "launch_ms"))
    cb = out.get("cpu_baseline") or {}
    if cb:
        line["cpu_baseline"] = pick(cb, ("value", "unit", "cores", "kind", "error"))
        if "sample" in cb:
            line["cpu_baseline"]["sample"] = cb["sample"].split(";")[0][:200]
        for twin in ("entry_twin", "poseidon_fixture"):
            if isinstance(cb.get(twin), dict):
                line["cpu_baseline"][twin] = pick(cb[twin], ("value", "unit", "cores", "ms_per_proof", "seconds", "kind", "error"))
    sr = out.get("step_resident") or {}
    if sr:
        line["step_resident"] = pick(sr, ("value", "unit", "ms_per_step"))
    pe = out.get("product_entry") or {}
    if pe:
        line["product_entry"] = pick(pe, ("ms_per_proof", "ms_per_proof_min_inner", "value", "proofs", "three_parties_agree", "plain_driver_ms", "error", "devices"))
        if isinstance(pe.get("shamir_party"), dict):
            line["product_entry"]["shamir_party_ms"] = _r(pe["shamir_party"].get("party_ms"))
    pf = out.get("poseidon_fixture") or {}
    if pf:
        line["poseidon_fixture"] = pick(pf, ("ms_per_proof", "ms_per_proof_min_inner", "value", "unit", "proofs", "three_parties_agree", "error"))
    if isinstance(out.get("sizes"), dict):
        line["sizes"] = {}
        for name, leg in out["sizes"].items():
            if "error" in leg:
                line["sizes"][name] = {"error": leg["error"][:120]}
            else:
                line["sizes"][name] = {"step_ms": _r(leg["step_resident"]["ms_per_step"]), "entry_ms": _r(leg["product_entry"]["ms_per_proof"]),
                                       "entry_value": _r(leg["product_entry"]["value"]), "roofline_frac": _r(leg["roofline"]["frac"]) if leg.get("roofline") else None}
    for name, leg in (out.get("session") or {}).items():
        if not isinstance(leg, dict) or not ({"step_resident", "product_entry"} <= set(leg) or "error" in leg):
            continue
        if "error" in leg:
            line.setdefault("second_curve", {})[name] = {"error": leg["error"][:120]}
        else:
            line.setdefault("second_curve", {})[name] = {"log_m": leg.get("log_m"), "step_ms": _r(leg["step_resident"]["ms_per_step"]), "entry_ms": _r(leg["product_entry"]["ms_per_proof"])}
    if "speedup_vs_cpu_baseline" in out:
        sp = out["speedup_vs_cpu_baseline"]
        line["speedup_vs_cpu_baseline"] = {k: _r(v) for k, v in sp.items()} if isinstance(sp, dict) else _r(sp)
    if isinstance(out.get("preflight"), dict):
        pf = out["preflight"]; pairs = [p for p in pf.get("pairs", []) if not p.get("same_gpu")]
        line["preflight"] = {"distinct_gpus": len({d["pci"] for d in pf.get("devices", [])}), "peer_pairs_checked": len(pairs), "pairs_without_peer_access": sum(1 for p in pairs if not p.get("peer_access")),
                             "min_pair_GBs": _r(min((p["GBs"] for p in pairs), default=None))}
    line["detail"] = detail_path
    text = json.dumps(line, separators=(",", ":"))
    for drop in ("second_curve", "sizes", "valu_roofline", "roofline_ntt", "roofline_g2", "speedup_vs_cpu_baseline"):     # never reached with today's legs; the limit is a contract
        if len(text) <= COMPACT_LIMIT:
            break
        line.pop(drop, None)
        text = json.dumps(line, separators=(",", ":"))
    assert len(text) <= COMPACT_LIMIT, len(text)
    return text


def emit(out, detail_path=None):
    """full object -> bench_detail.json (next to this script unless BENCH_DETAIL names another path), compact line -> stdout"""
    detail_path = detail_path or os.environ.get("BENCH_DETAIL") or os.path.join(ROOT, "bench_detail.json")
    try:
        with open(detail_path, "w") as f:
            json.dump(out, f, indent=1)
        shown = os.path.relpath(detail_path, ROOT) if detail_path.startswith(ROOT) else detail_path
    except OSError as e:
        shown = f"(not written: {e})"
    sys.stdout.write(compact_line(out, shown) + "\n")
    sys.stdout.flush()


def dump_outputs(dirname, arrays):
    """--dump-outputs: uint64 limb arrays -> DIR/<name>.npy as float64, each limb split into its two 32-bit words (low word first), which
    float64 holds exactly"""
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.uint64)
        np.save(os.path.join(dirname, name + ".npy"), a.view(np.uint32).reshape(a.shape[:-1] + (2 * a.shape[-1],)).astype(np.float64))


def cpu_baseline(log_m_target=22, threads_cap=None, budget_s=45.0):
    """oracle (C++ restatement of the reference path, arkworks' algorithms) timed on this host's cores on the SAME workload as the GPU
    line when the host manages it within the budget (2 x EPYC 9575F: 2^22 in ~35 s), else on the largest smaller domain that does.
    Two thread settings on the same inputs: all cores (capped at 64) and 15 = the ceil(254/17) windows arkworks' window-parallel MSM can
    keep busy at 2^22."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as orc
    cores = os.cpu_count() or 1
    threads = min(cores, threads_cap or 64)
    t_probe, _ = orc.bench_rep3_party(orc.BN254, 16, threads, seed=1)
    log_m = 16                                                         # time grows a little slower than m (wider MSM windows): 0.75 per doubling pair
    while log_m < log_m_target and t_probe * (1 << (log_m + 1 - 16)) * 0.75 <= budget_s:
        log_m += 1
    t15 = min(15, threads)
    (t, stages), (tb, stages_b), shared = orc.bench_rep3_party2(orc.BN254, log_m, threads, t15, seed=1)
    nc = (1 << log_m) - 2
    # CPU twins of the two figures the line leads with.  (i) `value` = the entry WITH the party's mask draws: the reference
    # draws 4 x m field elements per proof on one host thread inside mul_vec (rep3.rs:657-661, rngs.rs:37-46) — the resident workload above
    # plus exactly those draws.  (ii) the reference's own bench circuit (tests/benches/poseidon_hash2.rs:175-223 = the Poseidon fixture,
    # m = 256): one party on the zkey + wtns pair, draws included, best of three thread settings.
    twins = {}
    try:
        t_draws = orc.bench_mask_draws(orc.BN254, 1 << log_m)
        twins["entry_twin"] = {"value": nc / (t + t_draws), "unit": "constraints/s", "cores": threads, "kind": "port", "seconds": t + t_draws, "mask_draws_s": t_draws,
                               "what": f"the resident workload + the party's 4 x 2^{log_m} F::rand mask draws on one host thread as the reference makes them (rep3.rs:657-661, "
                                       "rngs.rs:37-46; scalar ChaCha12 restatement — rand_chacha's SIMD back end is faster, the product's own host draw takes "
                                       "product_entry.ms_per_proof_host_draws): the CPU twin of `value`; PCIe and serialisation have no CPU counterpart"}
    except Exception as e:                                                                   # noqa: BLE001
        twins["entry_twin"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    try:
        fxd = os.path.join(ROOT, "tests", "golden", "groth16", "bn254", "poseidon")
        best = None
        for th in sorted({1, min(8, threads), threads}):
            tp, stp = orc.bench_rep3_party_file(orc.BN254, os.path.join(fxd, "circuit.zkey"), os.path.join(fxd, "witness.wtns"), th, 10)
            if best is None or tp < best[0]:
                best = (tp, th, stp)
        twins["poseidon_fixture"] = {"ms_per_proof": best[0] * 1e3, "value": 213 / best[0], "unit": "constraints/s", "cores": best[1], "kind": "port", "stages_s": best[2],
                                     "what": "one REP3 party of the reference's bench circuit (Poseidon(2), 213 constraints, domain 256) on the host, mask draws included, "
                                             "best of 1 / 8 / all threads: the CPU twin of the `poseidon_fixture` leg"}
    except Exception as e:                                                                   # noqa: BLE001
        twins["poseidon_fixture"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    return {**twins, "value": nc / t, "unit": "constraints/s", "cores": threads, "kind": "port",
            "sample": f"one REP3 party's prove compute, synthetic BN254 R1CS m=2^{log_m} (the GPU line's config is m=2^{log_m_target}), {t:.2f} s wall with {threads} threads; "
                      "arkworks-algorithm restatement: window-parallel Pippenger (ark-ec msm_bigint, c=17 at 2^22: 15 windows = 15 busy threads), cache-blocked "
                      "data-parallel radix-2 FFT on a persistent thread pool, REP3 components processed one after the other (rep3.rs:942-943). EXCLUDED on both the "
                      "CPU and the GPU side: mask generation (rep3/rngs.rs:37-46: two ChaCha12 rejection-sampled field draws per element, the masks are inputs here), "
                      "serialisation and the network rounds of mul_vec, zkey parsing",
            "host_cores_total": cores, "stages_s": stages,
            "threads_15": {"value": nc / tb, "unit": "constraints/s", "cores": t15, "wall_s": tb, "stages_s": stages_b,
                           "note": "same inputs; " + ("both settings cover all 15 MSM windows, so the MSM stage times are shared and only the other stages were re-timed" if shared else "full second run")}}


def entry_leg(ctx, log_m, device, proofs, warmup, curve=None, extras=True, barrier=None, devices=None, files=None, outputs=None):
    """The product's entry under the driver's clock — what co-circom.rs:503-506 times: a proving session on a zkey FILE (product-side
    synthetic circuit with a valid CRS, cgh_synth_circuit) and ONE REP3 party through cgh_session_prove_rep3_party_ex, the entry the CLI
    patch binds.  Host buffers in, proof out: witness shares cross PCIe, the masks of both mul_vec calls are drawn INSIDE the call on the
    GPU from the party's two ChaCha12 generators (cgh_rep3_chacha; rep3/rngs.rs:37-46 makes them on one host thread), the vectors exchanged
    with the peers cross PCIe both ways.  The party is party 0 ALONE on the GPU, as in a deployment (one party per machine), served what its
    peers sent in a three-party run on the same session from page-locked memory: network time excluded; its proof must repeat bit for bit.
    Timed region = `proofs` consecutive calls between two barriers, wall clock.  extras: plain driver, the same party with host draws /
    pre-drawn masks, the Shamir twin.  devices: the party's GPUs — the session is then opened with cgh_session_open_multi over them (the product's
    multi-GPU path, SURVEY.md §8e: table slices per device, witness map distributed, partial sums folded on the host).  files = (zkey, wtns):
    an existing circuit instead of the synthetic one (log_m is then read from the zkey) — the reference's own bench circuit, Poseidon(2),
    tests/benches/poseidon_hash2.rs:175-223, is the fixture tests/golden/groth16/bn254/poseidon.  outputs (a dict): receives the last
    timed proof as "proof" (8 x words-per-field-element uint64: A, B, C affine)."""
    import shutil
    import tempfile
    import threading
    curve = CURVE if curve is None else curve
    devs = None if devices is None else [int(x) for x in devices]
    def sync_all():
        for dv in sorted(set(devs or [device.index])):
            torch.cuda.synchronize(dv)
        ctx.sync()
    barrier = barrier or sync_all
    d = tempfile.mkdtemp(prefix="cg_bench_")
    try:
        zp, wp = os.path.join(d, "s.zkey"), os.path.join(d, "s.wtns")
        t_gen = 0.0
        if files is not None:
            zp, wp = files
        else:
            t0 = time.perf_counter(); cg.host_synth_circuit(curve, log_m, 0xC0C1C0DE, zp, wp, device=device.index); t_gen = time.perf_counter() - t0
        pre = int(os.environ["BENCH_PRECOMPUTE"]) if os.environ.get("BENCH_PRECOMPUTE") else True      # A/B knob (scripts/): window of the precomputed tables, 0 = none
        t0 = time.perf_counter(); ses = cg.ProvingSession(curve, zp, precompute=pre, device=device.index, devices=devs, shared_devices=bool(devs) and len(set(devs)) < len(devs)); t_open = time.perf_counter() - t0
        zkey_bytes = os.path.getsize(zp)
        w = cg.host_read_wtns(curve, wp)
        info = cg.host_zkey_info(curve, zp)
        n_in = info["n_public"] + 1                          # the leading one + the public inputs
        m, log_m, nc, n_aux = info["domain_size"], info["pow"], info["num_constraints"], w.shape[0] - n_in
        g = torch.Generator(device=device); g.manual_seed(0x5E55)
        host = lambda t: t.cpu().numpy().view(np.uint64)
        # additive shares of the aux witness: a, b uniform, c = w - a - b (on the device, through the ABI's own subtraction)
        da, db = rand_fr(n_aux, device, g, curve), rand_fr(n_aux, device, g, curve)
        dw = torch.from_numpy(np.ascontiguousarray(w[n_in:]).view(np.int64)).to(device)
        dc = torch.empty_like(dw)
        ctx.vec_sub(curve, dc, dw, da, n_aux); ctx.vec_sub(curve, dc, dc, db, n_aux); ctx.sync(); torch.cuda.synchronize()
        pin = lambda x: (lambda p_: (p_.__setitem__(slice(None), x), p_)[1])(ctx.host_alloc(x.shape))
        a, b, c = pin(host(da)), pin(host(db)), pin(host(dc))
        del da, db, dc, dw
        wa, wb = [a, b, c], [c, a, b]
        pinned = [a, b, c]
        out = {"entry": "cgh_session_prove_rep3_party_ex (host buffers in, proof out; network and randomness through the callback tables, cgh_rep3_chacha: "
                        "generators described by seed + word position)", "log_m": log_m, "curve": CURVE_NAME[curve], "pcie_inclusive": True,
               "devices": devs or [device.index], "session": "cgh_session_open_multi over %d device(s)" % len(devs or [0]),
               "circuit": dict(info, source=("file " + os.path.relpath(zp, ROOT)) if files is not None else "synthetic (cgh_synth_circuit, seed 0xC0C1C0DE)"),
               "network": "loopback replay from page-locked memory (excluded, SURVEY.md 8d)",
               "randomness": "4 x m ChaCha12 / F::rand masking draws per proof INSIDE the timed call, on the GPU (cg_chacha12_fr_rand_dev); draw order restated from "
                             "rand_chacha 0.3 / ark-ff 0.4.2: parity unpinned (no reference-held vector exists)"}
        # Three parties, one thread each, every one through the ONE-PARTY entry; the transport is the in-process loopback, party 0's incoming
        # traffic is recorded.
        seeds = [bytes((37 * i + 11 * k + 5) & 255 for k in range(32)) for i in range(3)]

        def three_parties(record):
            hub = cg.LoopbackHub()
            rnd = [cg.ChaChaRand(curve, seeds[i], seeds[(i + 2) % 3]) for i in range(3)]
            nets = [hub.net(i, record=(record and i == 0)) for i in range(3)]
            res, errs = [None] * 3, [None] * 3

            def party(i):
                try: res[i], _ = cg.host_prove_rep3_party(ses, w[:n_in], wa[i], wb[i], nets[i], rnd[i].table, rnd[i].streams)
                except Exception as e: errs[i] = e; hub.abort()
            th = [threading.Thread(target=party, args=(i,)) for i in range(3)]
            t0 = time.perf_counter()
            for t in th: t.start()
            for t in th: t.join()
            dt = time.perf_counter() - t0
            for r_ in rnd: r_.close()
            if any(errs): raise RuntimeError(f"REP3 parties failed: {errs}")
            return hub, np.stack(res), dt
        hub, _, _ = three_parties(False); hub.close()                                   # warm-up (scratch arenas, twiddles, page-locked rings)
        hub, proofs3, t_three = three_parties(True)
        out["three_parties_agree"] = bool((proofs3[0] == proofs3[1]).all() and (proofs3[1] == proofs3[2]).all())
        out["rep3_three_parties_one_gpu_ms"] = t_three * 1e3

        def solo(on_device=True, prepared=None):
            # the party's network and Rep3Rand exist before the reference starts its clock (co-circom.rs:484-502 set them up, :503-506 time prove)
            rnd, net = prepared or (cg.ChaChaRand(curve, seeds[0], seeds[2]), hub.replay_net(0))
            got, sec = cg.host_prove_rep3_party(ses, w[:n_in], wa[0], wb[0], net, rnd.table, rnd.streams if on_device else None)
            if prepared is None:
                rnd.close()
                if not (got == proofs3[0]).all(): raise RuntimeError("the party served its recorded traffic produced a different proof")
            return (got, sec) if prepared else sec
        for _ in range(warmup):
            solo()
        prepared = [(cg.ChaChaRand(curve, seeds[0], seeds[2]), hub.replay_net(0)) for _ in range(proofs)]
        # (the interpreter's cyclic garbage collector is held off the timed region, as timeit does: with torch loaded one full collection takes
        # ~40 ms, and when it fell into the ten 4 ms proofs of a 2^16 leg that leg read 8.8 ms per proof with 4.6 ms inside every call)
        gc.collect(); gc.disable()
        try:
            barrier()
            t0 = time.perf_counter()
            timed = [solo(prepared=pr) for pr in prepared]
            barrier()
            elapsed = time.perf_counter() - t0
        finally:
            gc.enable()
        for rnd_, _ in prepared: rnd_.close()
        if not all((got == proofs3[0]).all() for got, _ in timed): raise RuntimeError("the party served its recorded traffic produced a different proof")
        inner = [sec for _, sec in timed]
        if outputs is not None:
            outputs["proof"] = timed[-1][0].copy()
        out.update({"proofs": proofs, "warmup": warmup, "elapsed_s": elapsed, "ms_per_proof": elapsed / proofs * 1e3, "ms_per_proof_min_inner": min(inner) * 1e3, "ms_per_proof_mean_inner": sum(inner) / len(inner) * 1e3, "ms_inner_each": [round(x * 1e3, 1) for x in inner],
                    "value": nc / (elapsed / proofs), "unit": "constraints/s"})
        if extras:
            try:                                                                         # the reference's way: the same generators drawn on one host thread inside the call
                out["ms_per_proof_host_draws"] = solo(False) * 1e3
            except Exception as e:                                                       # noqa: BLE001 (a secondary figure must not take the bench line down)
                out["ms_per_proof_host_draws"] = None; out["host_draws_error"] = str(e)[:200]
            try:
                r, s_ = host(rand_fr(2, device, g, curve))
                ses.prove_plain(w, r, s_)
                plain = [ses.prove_plain(w, r, s_)[1] for _ in range(3)]
                out["plain_driver_ms"] = min(plain) * 1e3
                out["plain_driver_constraints_per_s"] = nc / min(plain)
            except Exception as e:                                                       # noqa: BLE001
                out["plain_driver_error"] = str(e)[:200]
        hub.close()
        # The Shamir twin (co-circom.rs:507-527), t = 1 of 3: three seeded parties over the library's in-memory mesh, then party 1 (and the king)
        # ALONE on the GPU with the received messages replayed; preprocess of 2 m / (t + 1) secrets (its draws on the GPU) inside the call.
        if extras:
            try:
                dr = rand_fr(n_aux, device, g, curve)
                dw = torch.from_numpy(np.ascontiguousarray(w[n_in:]).view(np.int64)).to(device)
                swits, cur = [], dw
                for _ in range(3):                                                          # w + r x at x = 1, 2, 3 (shamir_core.rs:8-31)
                    nxt = torch.empty_like(dw); ctx.vec_add(curve, nxt, cur, dr, n_aux); ctx.sync(); torch.cuda.synchronize()
                    swits.append(pin(host(nxt))); cur = nxt
                pinned += swits
                del dr, dw, cur, nxt
                pre = (2 * m + 8) // 2 + 1
                sseeds = [bytes((29 * i + 13 * k + 3) & 255 for k in range(32)) for i in range(3)]
                hubs = cg.ShamirLoopbackHub(3)
                snets = [hubs.net(i, record=True) for i in range(3)]
                souts, serrs = [None] * 3, [None] * 3

                def party_s(i):
                    try: souts[i], _ = cg.host_prove_shamir_party_seeded(ses, 1, w[:n_in], swits[i], snets[i], sseeds[i], preprocess=pre)
                    except Exception as e: serrs[i] = e; hubs.abort()
                th = [threading.Thread(target=party_s, args=(i,)) for i in range(3)]
                t0 = time.perf_counter()
                for t in th: t.start()
                for t in th: t.join()
                t3 = time.perf_counter() - t0
                if any(serrs): raise RuntimeError(f"Shamir parties failed: {serrs}")
                alone = {}
                for i in (1, 0):
                    secs = []
                    for _ in range(3):
                        got, sec = cg.host_prove_shamir_party_seeded(ses, 1, w[:n_in], swits[i], hubs.replay_net(i), sseeds[i], preprocess=pre)
                        if not (got == souts[0]).all(): raise RuntimeError("Shamir: replayed party produced a different proof")
                        secs.append(sec * 1e3)
                    alone[i] = secs
                hubs.close()
                out["shamir_party"] = {"entry": "cgh_session_prove_shamir_party_seeded (t = 1 of 3; the party's generator seeded by the caller, its draws on the GPU)",
                                       "party_ms": sum(alone[1]) / 3, "party_ms_min": min(alone[1]), "king_ms": sum(alone[0]) / 3, "three_parties_one_gpu_ms": t3 * 1e3,
                                       "party_constraints_per_s": nc / (sum(alone[1]) / 3 * 1e-3), "preprocess_secrets": pre, "draws_on_gpu": pre * 4,
                                       "three_parties_agree": bool((souts[0] == souts[1]).all() and (souts[1] == souts[2]).all()),
                                       "note": "one party alone on the GPU, the messages it received replayed from page-locked memory (network excluded); preprocessing, both "
                                               "degree reductions and every message crossing PCIe inside the timed call"}
            except Exception as e:                                                          # noqa: BLE001
                out["shamir_party"] = {"error": str(e)[:300]}
        ses.close()
        for x in pinned:
            ctx.host_free(x)
        out["zkey"] = {"generate_s": t_gen, "session_open_s": t_open, "file_bytes": zkey_bytes,
                       "note": "untimed, like the reference's zkey parse (co-circom.rs:482 precedes the Instant at :503); session_open = map + decode the file, upload, "
                               "validate every point on the GPU (on-curve + subgroup), precompute the window tables"}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def session_leg(ctx, log_m, device, proofs=5, warmup=1, curve=None):
    """scripts/: the entry leg alone (A/B runs of host-side scheduling knobs, other sizes)"""
    return entry_leg(ctx, log_m, device, proofs, warmup, curve=curve)


def timed_resident_steps(w, ctxs, steps, warmup, run_step, barrier, comm):
    """W untimed + exactly K timed resident steps between two barriers; returns (seconds, merged stage statistics, last results)"""
    res = None
    for _ in range(warmup):
        res = run_step()
    # The timed steps run with the library's statistics OFF: a statistics span is a pair of timing events created and recorded around every
    # launch sequence (~100 pairs per step), and a later leg of the same process found part of them pooled and part not — the 2^20 step
    # measured 19.9 ms after a 20-step main leg and 23-28 ms after a 5-step one.  The per-stage figures come from an untimed pass behind.
    stats_in_timed = bool(os.environ.get("BENCH_STATS_IN_TIMED"))                       # A/B knob: the rounds 1-4 arrangement
    if stats_in_timed:
        for c in ctxs:
            c.stats_enable(True); c.stats(reset=True)
    gc.collect(); gc.disable()                                                          # (see entry_leg)
    try:
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            res = run_step()
        barrier()
        elapsed = comm.max_float(time.perf_counter() - t0)
    finally:
        gc.enable()
    stat_steps = steps
    if not stats_in_timed:
        stat_steps = max(2, min(steps, 5))
        for c in ctxs:
            c.stats_enable(True); c.stats(reset=True)
        for _ in range(stat_steps):
            res = run_step()
        barrier()
    st = None
    for c in ctxs:
        s_ = c.stats(reset=True); c.stats_enable(False)
        st = s_ if st is None else {k: st[k] + s_[k] for k in st}
    if stat_steps != steps:                                                             # totals are read per timed step by the callers
        st = {k: (v * steps / stat_steps if k.endswith("_ms") else int(round(v * steps / stat_steps))) for k, v in st.items()}
    return elapsed, st, res


def isolated_kernels(w, ctx, barrier, reps=3):
    """The kernels on their own (untimed): one share component at a time on one context, so that the digit/sort schedule, the accumulation
    and the bucket reduction run one after the other and nothing shares the CUs — the per-launch figures rocprofv3 lists for a serial run
    (profiles/r0N_serial_kernel_stats.csv).  HIP events of the library on the kernels' own streams."""
    def alone(fn):
        fn(); barrier()
        ctx.stats_enable(True); ctx.stats(reset=True)
        for _ in range(reps):
            fn()
        barrier()
        st_ = ctx.stats(reset=True); ctx.stats_enable(False)
        return st_
    iso = {}
    g1_key = next((k for k in w.tables if TABLE_GROUP[k[0]] == 0), None)
    g2_key = next((k for k in w.tables if TABLE_GROUP[k[0]] == 1), None)
    for name, key in (("g1", g1_key), ("g2", g2_key)):
        if key is None:
            continue
        bases, lo, hi = w.tables[key]
        sc = [(w.ha if key[0] == "h" else w.wa)[lo:hi]]
        st_ = alone(lambda: ctx.msm_end(ctx.msm_dev_begin_multi([bases], sc, hi - lo)[0]))
        iso["acc_%s_ms" % name] = st_["msm_acc_%s_ms" % name] / max(1, st_["msm_acc_%s_calls" % name])
        iso["sort_ms"] = st_["msm_sort_ms"] / reps
        iso["reduce_%s_ms" % name] = st_["msm_reduce_ms"] / reps
        iso["points_%s" % name] = hi - lo
    st_ = alone(lambda: ctx.ntt_dev(w.curve, [w.ca], w.m, w.omega))
    iso["ntt_ms"] = st_["ntt_ms"] / reps
    st_ = alone(lambda: ctx.ntt_coset_pair_dev(w.curve, [w.ca], w.m, w.omega, w.coset_g))
    iso["ntt_pair_ms"] = st_["ntt_ms"] / reps                                # iNTT + coset shift + NTT of one vector as the step runs them
    st_ = alone(lambda: (ctx.spmv_csr(w.curve, w.rpA, w.colA, w.coA, w.nc, w.pub, w.n_inputs, 0, w.wa, w.wb, w.aa, w.ab),
                         ctx.spmv_csr(w.curve, w.rpB, w.colB, w.coB, w.nc, w.pub, w.n_inputs, 0, w.wa, w.wb, w.ba, w.bb)))
    iso["spmv_pair_ms"] = st_["spmv_ms"] / reps
    st_ = alone(lambda: ctx.vec_rep3_mul_local(w.curve, w.ca, w.aa, w.ab, w.ba, w.bb, w.mask1, w.m))
    iso["rep3_mul_local_ms"] = st_["vec_ms"] / reps
    return iso


def measure_acc_traffic(log_m, timeout_s=150):
    """HBM bytes per launch of the dominant kernel, measured NOW: two rocprofv3 passes (--pmc FETCH_SIZE, then --pmc WRITE_SIZE, each with
    --kernel-trace only: MI355X_MICROARCH.md's recipe) over scripts/acc_traffic.py, which runs the same accumulation alone.  The counters
    come in KiB; FETCH_SIZE under-reports this kernel's scattered 64-byte gathers by the factor calibrated on known byte counts in
    profiles/r04_pmc_calibration.json (gather64_read), WRITE_SIZE needs none.  Returns (bytes, note) or (None, why not)."""
    import csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 is not on PATH"
    if os.environ.get("BENCH_NO_PMC") or any(k.startswith("ROCPROF") or k.startswith("ROCP_") for k in os.environ):
        return None, "skipped (BENCH_NO_PMC set, or this process already runs under a profiler)"
    try:
        with open(os.path.join(ROOT, "profiles", "r04_pmc_calibration.json")) as f:
            cal = json.load(f)["true_bytes_over_counter_bytes"]
    except Exception:                                                                        # noqa: BLE001
        cal = {"gather64_read": 1.0, "dword_write": 1.0}
    total, parts = 0.0, {}
    d = tempfile.mkdtemp(prefix="cg_pmc_")
    try:
        for counter, factor in (("FETCH_SIZE", cal.get("gather64_read", 1.0)), ("WRITE_SIZE", cal.get("dword_write", 1.0))):
            out = os.path.join(d, counter)
            env = dict(os.environ, TMPDIR="/tmp")
            p = subprocess.run([exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "--", sys.executable,
                                os.path.join(ROOT, "scripts", "acc_traffic.py"), str(log_m), "2"], cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            if p.returncode != 0:
                return None, f"rocprofv3 --pmc {counter} failed (rc {p.returncode}): {p.stderr[-200:]}"
            vals = []
            for fcsv in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(fcsv)):
                    if "k_msm_accumulate_pf" in r.get("Kernel_Name", "") and r.get("Counter_Name") == counter:
                        vals.append(float(r["Counter_Value"]))
            if not vals:
                return None, f"no {counter} rows for k_msm_accumulate_pf in the counter collection"
            # one row per dispatch (summed over the XCDs by the tool) or one per (dispatch, dimension): sum, then per launch (2 launches)
            per_launch = sum(vals) / 2.0 * 1024.0 * factor
            parts[counter] = per_launch; total += per_launch
        return total, ("measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE (two passes) over scripts/acc_traffic.py; read %.3g B x gather calibration %.3f "
                       "(profiles/r04_pmc_calibration.json) + written %.3g B per launch" % (parts["FETCH_SIZE"], cal.get("gather64_read", 1.0), parts["WRITE_SIZE"]))
    except Exception as e:                                                                   # noqa: BLE001 (a side figure must not take the line down)
        return None, f"{type(e).__name__}: {e}"[:300]
    finally:
        shutil.rmtree(d, ignore_errors=True)


def roof(bytes_, ms, **extra):
    if not ms:
        return None
    r = {"bound": "hbm", "achieved": bytes_ / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bytes_ / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
         "launch_ms": ms, "algorithmic_bytes_per_launch": bytes_}
    r.update(extra)
    return r


def stage_table(iso, k=2):
    """per-stage ms of one step from the ISOLATED launches x the launches a step makes (what replaced the event spans across overlapped
    streams, which summed to four times the step): the sum is the serial kernel time of a step; the step itself overlaps the stages"""
    if not iso or "acc_g1_ms" not in iso:
        return None
    rows = {"spmv": (iso.get("spmv_pair_ms", 0.0), 1, "2 constraint mat-vecs"),
            "rep3_mul_local": (iso.get("rep3_mul_local_ms", 0.0), 2, "masked local products of the two mul_vec calls"),
            "ntt_pair": (iso["ntt_pair_ms"], 3 * k, "iNTT + coset shift + NTT per vector: a, b, c x %d share components" % k),
            "msm_sort": (iso["sort_ms"], 2 * k, "digit + sort schedule per scalar vector: aux and h shares"),
            "msm_acc_g1": (iso["acc_g1_ms"], 4 * k, "bucket accumulation h, l, a, b1"),
            "msm_acc_g2": (iso.get("acc_g2_ms", 0.0), k, "bucket accumulation b2"),
            "msm_reduce_g1": (iso["reduce_g1_ms"], 4 * k, "merge of chunk-boundary pieces + bucket reduction"),
            "msm_reduce_g2": (iso.get("reduce_g2_ms", 0.0), k, "merge of chunk-boundary pieces + bucket reduction")}
    out = {name: {"isolated_ms": ms, "launches_per_step": n, "ms_per_step": ms * n, "what": what} for name, (ms, n, what) in rows.items()}
    out["serial_sum_ms"] = sum(v["ms_per_step"] for v in out.values())
    return out


def window_of(points, precompute):
    return (20 if points > (3 << 20) else 16 if points <= (1 << 18) else 17) if precompute < 0 else (precompute or 16)


def resident_leg(ctx, ctx_aux, device, log_m, steps, warmup, curve, precompute=-1, scatter_cap=-1):
    """the inputs-resident step at one size on one GPU with its isolated launches and roofline triple (the `sizes` / BLS legs)"""
    w = Workload(ctx, log_m, device, 0, 1, precompute=precompute, curve=curve)
    w.emulate, w.g2_last, w.comm, w.pcie, w.ctx_aux = False, False, Comm(None, 1, device), None, ctx_aux
    try:
        def barrier():
            torch.cuda.synchronize(); ctx.sync()
            if ctx_aux is not None:
                ctx_aux.sync()
        elapsed, st, _ = timed_resident_steps(w, [c for c in (ctx, ctx_aux) if c is not None], steps, warmup, lambda: exchange(step(w), w.plan, w.comm, curve), barrier, w.comm)
        iso = isolated_kernels(w, ctx, barrier)
        ptb = G1_POINT_BYTES[curve]
        out = {"ms_per_step": elapsed / steps * 1e3, "value": w.nc / (elapsed / steps), "unit": "constraints/s", "steps": steps, "warmup": warmup,
               "roofline": roof((ptb + 32.0) * iso["points_g1"], iso["acc_g1_ms"], kernel="k_msm_accumulate_pf<G1>"),
               "roofline_g2": roof((2 * ptb + 32.0) * iso["points_g2"], iso.get("acc_g2_ms"), kernel="k_msm_accumulate_pf<G2>"),
               "roofline_ntt": roof(64.0 * w.m, iso["ntt_ms"], kernel="one 2^%d transform" % log_m),
               "isolated_ms": iso, "stages": stage_table(iso),
               "step_hbm": {"algorithmic_bytes_per_step": 2048.0 * w.nc, "achieved_GBs": 2048.0 * w.nc / (elapsed / steps) / 1e9, "frac": 2048.0 * w.nc / (elapsed / steps) / 1e9 / HBM_PEAK_GBS}}
        # SURVEY §8d "also report achieved 32-bit mul-add rate": every point is added once per window
        nw = lambda pts: FR[curve][2] // window_of(pts, precompute) + 1
        valu = {}
        for name, mads in (("g1", MADS_PER_G1_ADD[curve]), ("g2", MADS_PER_G2_ADD[curve])):
            ms, pts = iso.get("acc_%s_ms" % name), iso.get("points_%s" % name)
            if ms and pts:
                rate = mads * pts * nw(pts) / (ms * 1e-3) / 1e12
                valu[name] = {"mads_per_point_addition": mads, "achieved_Tmad_s": rate, "peak_Tmad_s": MAD_PEAK_T, "frac": rate / MAD_PEAK_T, "launch_ms": ms}
        out["valu_roofline"] = valu
        return out
    finally:
        w.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-m", type=int, default=22)
    ap.add_argument("--curve", default="bn254", choices=["bn254", "bls12_381"], help="curve of the line (the BASELINE metric is BN254; bls12_381 = the second curve of the reference's e2e matrix)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-session", action="store_true", help="skip the entry legs (the product's file -> proof entry): `value` is then the inputs-resident step (value_basis says so)")
    ap.add_argument("--no-sizes", action="store_true", help="skip the legs at the other north_star sizes (2^16, 2^20, 2^24) and on the second curve")
    ap.add_argument("--sizes", default="16,20,24", help="log2 domain sizes of the `sizes` legs")
    ap.add_argument("--scatter-cap", type=int, default=-1, help="-1 = exact two-pass sort (default), 0 = optimistic one-pass scatter (auto capacity)")
    ap.add_argument("--g2-last", action="store_true", help="experiment: put the G2 table last in the multi-table MSM")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend (gloo: test mode, exchanges staged through the host)")
    ap.add_argument("--shared-device", action="store_true", help="test mode: every rank uses GPU 0 (several ranks on one GPU; needs --backend gloo)")
    ap.add_argument("--dump-result", default=None, help="rank 0 writes the five folded MSM results (affine) of the last step to this .npz")
    ap.add_argument("--dump-inputs", action="store_true", help="with --dump-result: also store the step's inputs (small --log-m only; tests check the results against the oracle)")
    ap.add_argument("--emulate", default=None, metavar="WORLD:RANK", help="planner tuning: time ONLY the work the plan gives RANK of WORLD, on this one GPU, "
                    "with the exchanges skipped (results are not folded; not a benchmark line)")
    ap.add_argument("--pcie", action="store_true", help="resident step + what a real REP3 party moves over PCIe every step - witness shares, the two masks and the two "
                    "received vectors up, the two local products down (the entry legs measure the real thing)")
    ap.add_argument("--soak", type=int, default=0, metavar="K", help="after the timed region run K more (untimed) steps and require every one of them to reproduce "
                    "the folded results of the last timed step bit for bit (the inputs are the same each step: a race between the streams shows up as a mismatch)")
    ap.add_argument("--force-dist", action="store_true", help="test mode: initialise torch.distributed even for one rank and distribute the witness map from "
                    "one rank on, so that a single GPU drives the RCCL all_to_all / all_gather / all_reduce calls of the N >= 4 path")
    ap.add_argument("--one-context", action="store_true", help="run the aux-witness MSMs after the witness map on the same context (no overlap)")
    ap.add_argument("--precompute", type=int, default=-1, help="window size of the per-window precomputed base tables (-1 = by table size: 20 above ~3 M G1 / ~1.5 M G2 points else 17; 0 = off)")
    ap.add_argument("--full", action="store_true", help="everything beside the headline: for N = 1 the resident step with its isolated launches, rooflines and copy "
                    "ceiling, the entry's extras (host draws, plain driver, Shamir twin), the `sizes` legs, the Poseidon fixture, the second curve, the in-run "
                    "counter passes and the CPU baseline (--no-sizes / --no-cpu-baseline still drop theirs).  Without it an N = 1 run times the headline only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps write what the timed path handed its caller in the last step "
                    "as DIR/<name>.npy, float64: the proof's affine points A, B, C of the entry (or the folded MSM results of the resident step when that "
                    "is the headline), each 64-bit limb split into two 32-bit words, low word first")
    args = ap.parse_args()
    global CURVE
    CURVE = cg.BN254 if args.curve == "bn254" else cg.BLS12_381

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    emulate = None
    if args.emulate:
        emulate = tuple(int(x) for x in args.emulate.split(":"))
    # `python bench.py --gpus N` with no launcher around it (the driver's N = 1 command shape): start the N ranks here, one per GPU, under
    # torch.distributed.run — and refuse loudly when the box has fewer GPUs than ranks (test mode --shared-device puts every rank on GPU 0).
    # The launcher is a child process: this process has already opened the GPU (the checks above), and replacing such a process with
    # exec is not safe on every driver.
    if "WORLD_SIZE" not in os.environ and args.gpus > 1 and not emulate:
        have = torch.cuda.device_count()
        if have < args.gpus and not args.shared_device:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible (one rank per GPU; --shared-device --backend gloo is the one-GPU test mode)")
        import socket
        import subprocess
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.stdout.flush(); sys.stderr.flush()
        p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
                            "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:])
        sys.exit(p.returncode if p.returncode >= 0 else 128 - p.returncode)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and not (emulate and world == 1):
        raise SystemExit(f"bench.py --gpus {args.gpus} was started with WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus} (or without a launcher: bench.py starts its own ranks)")
    if world > 1 and not args.shared_device and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: {world} ranks but only {torch.cuda.device_count()} GPU(s) visible")
    if args.shared_device:
        local_rank = 0
    if emulate:
        assert world == 1, "--emulate runs as a single process"
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    host_group = None                                  # host-side barrier (gloo): a waiting rank must not spin a kernel on its GPU while rank 0's session uses that GPU
    if args.force_dist:
        global WM_DISTRIBUTE_MIN_WORLD
        WM_DISTRIBUTE_MIN_WORLD = 1
        os.environ.setdefault("MASTER_PORT", "29655"); os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
    ranks_seen = 1
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # (gloo announces its connections on STDOUT from C++: the line this script prints must stay the only thing there, so the
        # descriptor points at stderr while the process groups are made)
        sys.stdout.flush(); saved_out = os.dup(1); os.dup2(2, 1)
        try:
            if args.backend == "nccl":
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
                host_group = dist.new_group(backend="gloo")
            else:
                dist.init_process_group("gloo", rank=rank, world_size=world)
            dist.barrier(group=host_group) if host_group is not None else dist.barrier()
        finally:
            sys.stdout.flush(); os.dup2(saved_out, 1); os.close(saved_out)
        ones = torch.ones(1, dtype=torch.int64, device=device if args.backend == "nccl" else None)
        dist.all_reduce(ones)                              # every rank of the job answered through the data-path backend (nccl = RCCL)
        ranks_seen = int(ones.item())
        if ranks_seen != world:
            raise SystemExit(f"bench.py: all_reduce of ones over {world} ranks returned {ranks_seen}")
    # N > 1, first contact with the node: N DISTINCT GPUs that reach each other over peer copies (cg_device_preflight: PCI bus ids, peer access,
    # one checked 1 MiB copy per ordered pair), or no number is printed.  --shared-device (the one-GPU test mode) allows the repeats and says so.
    preflight = None
    if world > 1 and rank == 0:
        devs = [0] * world if args.shared_device else list(range(world))
        preflight = cg.device_preflight(devs, allow_shared=args.shared_device, allow_staged=True)
        pairs = [p for p in preflight["pairs"] if not p["same_gpu"]]
        if any(not p["peer_access"] for p in pairs):
            print("bench.py preflight: WARNING — " + ", ".join(f"{p['src']}->{p['dst']}" for p in pairs if not p["peer_access"]) +
                  " have NO peer access: device-to-device copies are staged through the host (not xGMI)", file=sys.stderr)
        print(f"bench.py preflight: {len(set(d['pci'] for d in preflight['devices']))} distinct GPU(s) for {world} rank(s), {len(pairs)} peer pairs checked"
              + (f", slowest 1 MiB copy {min(p['GBs'] for p in pairs):.1f} GB/s" if pairs else " (shared-device test mode)"), file=sys.stderr)
    comm = Comm(dist, world, device)

    ctx = cg.Context(local_rank)
    stream = torch.cuda.Stream(device=device)      # torch is plumbing: one stream shared by its copies/slices and the library's kernels
    ctx.set_stream(stream.cuda_stream)
    torch.cuda.set_stream(stream)
    ctx.set_scatter_capacity(args.scatter_cap)
    # The inputs-resident step: the headline with --no-session, the strong-scaling figure of N > 1, and what the resident-step options act on.
    # A plain N = 1 run leads with the product entry and leaves it to --full.
    resident = (args.full or args.no_session or world > 1 or emulate is not None or args.force_dist or args.one_context or args.g2_last or args.pcie
                or bool(args.soak) or args.dump_result is not None)
    w = None
    if resident:
        w = Workload(ctx, args.log_m, device, emulate[1] if emulate else rank, emulate[0] if emulate else world, precompute=args.precompute)
        w.emulate = emulate is not None
        w.g2_last = args.g2_last
        w.comm = comm
        w.pcie = None
        if args.pcie:
            pin = lambda t: torch.empty(t.shape, dtype=t.dtype).pin_memory().copy_(t.cpu())
            w.pcie = {"up": [(getattr(w, k), pin(getattr(w, k))) for k in ("wa", "wb", "mask1", "mask2", "recv1", "recv2")],
                      "down": [(getattr(w, k), pin(getattr(w, k))) for k in ("ca", "ha")]}
        w.ctx_aux = None
        if not args.one_context:
            w.ctx_aux = cg.Context(local_rank)
            w.ctx_aux.set_scatter_capacity(args.scatter_cap)
    torch.cuda.synchronize()

    def barrier():
        torch.cuda.synchronize(); ctx.sync()
        if w is not None and w.ctx_aux is not None:
            w.ctx_aux.sync()
        if dist is not None:
            dist.barrier()

    if resident:
        run_step = (lambda: step(w)) if emulate else (lambda: exchange(step(w), w.plan, comm, CURVE))
        elapsed, st, res = timed_resident_steps(w, [c for c in (ctx, w.ctx_aux) if c is not None], args.steps, args.warmup, run_step, barrier, comm)

    if args.soak and not emulate:
        ref = {t: np.array(v, copy=True) for t, v in res.items()}
        for it in range(args.soak):
            again = run_step()
            for t in ref:
                for j in range(2):
                    same = np.array_equal(cg.point_to_affine(CURVE, cg.G1 if TABLE_GROUP[t] == 0 else cg.G2, ref[t][j]),
                                          cg.point_to_affine(CURVE, cg.G1 if TABLE_GROUP[t] == 0 else cg.G2, again[t][j]))
                    if not same:
                        raise SystemExit(f"soak: step {it} produced a different result for table {t} component {j} (rank {rank})")
        barrier()
        if rank == 0:
            print(f"soak: {args.soak} extra steps reproduced the results bit for bit", file=sys.stderr)

    single = rank == 0 and not emulate and world == 1
    iso = isolated_kernels(w, ctx, barrier) if single and args.full else None
    g1_pts = [hi - lo for (t, i, parts), (b, lo, hi) in w.tables.items() if TABLE_GROUP[t] == 0] if resident else []
    folded = None                                      # the resident step's results as its caller gets them: affine points, table -> (2 components, words)
    if resident and rank == 0 and not emulate:
        folded = {t: np.stack([cg.point_to_affine(CURVE, cg.G1 if TABLE_GROUP[t] == 0 else cg.G2, res[t][j]) for j in range(2)]) for t in TABLES}

    if rank == 0 and args.dump_result:
        dump = dict(folded)
        if args.dump_inputs:
            u64 = lambda t: t.cpu().numpy().view(np.uint64) if t.dtype == torch.int64 else t.cpu().numpy()
            for name in ("rpA", "colA", "coA", "rpB", "colB", "coB", "pub", "wa", "wb", "mask1", "mask2", "recv1", "recv2"):
                dump["in_" + name] = u64(getattr(w, name))
            dump["in_omega"], dump["in_coset_g"] = w.omega, w.coset_g
            dump["in_shape"] = np.array([w.m, w.nc, w.n_inputs, w.n_aux], dtype=np.int64)
        np.savez(args.dump_result, **dump)
    if emulate:
        print(json.dumps({"emulated_world": emulate[0], "emulated_rank": emulate[1], "ms_per_step": elapsed / args.steps * 1e3,
                          "units": [f"{t}{i}/{p}" for (t, i, p) in w.mine], "vectors": w.my_vecs, "stage_ms": {k: v / args.steps for k, v in st.items() if k.endswith("_ms")}}))
        return
    # N > 1: the SAME basis as the N = 1 line — one REP3 party through the product's entry, on a session opened over the job's N GPUs
    # (cgh_session_open_multi: one process drives the party's devices, as one `co-circom` process would).  Rank 0 is that process; the
    # other ranks have done their part in the resident leg above and wait in a HOST-side barrier, their GPUs free for the session.
    multi_ent = None
    entry_out = {}                                     # the headline entry's last timed proof (entry_leg's `outputs`)
    if world > 1 and not emulate and not args.no_session:
        w.release()
        for c in (w.ctx_aux, ctx):                    # the waiting ranks give their contexts back: rank 0's session is alone on the job's GPUs
            if c is not None and rank != 0:
                c.close()
        host_barrier = (lambda: dist.barrier(group=host_group)) if host_group is not None else dist.barrier
        torch.cuda.synchronize(); host_barrier()
        if rank == 0:
            devs = [0] * world if args.shared_device else list(range(world))
            try:
                multi_ent = entry_leg(ctx, args.log_m, device, args.steps, args.warmup, CURVE, extras=False, devices=devs, outputs=entry_out)
            except Exception as e:                                                       # noqa: BLE001 (the line survives: `value` stays the resident step and says so)
                multi_ent = {"error": f"{type(e).__name__}: {e}"[:400], "devices": devs}
        host_barrier()
    if rank == 0 and resident:
        step_ms = elapsed / args.steps * 1e3
        step_value = w.nc / (elapsed / args.steps)
        ptb = G1_POINT_BYTES[CURVE]
        # dominant kernel: G1 bucket accumulation. Algorithmic bytes per launch: each base read once (64 B; 96 B on BLS12-381)
        # + its scalar read once (32 B) per point of the launch's range.
        acc_calls = max(1, st["msm_acc_g1_calls"])
        avg_ms = st["msm_acc_g1_ms"] / acc_calls
        avg_pts = (sum(g1_pts) / len(g1_pts)) if g1_pts else 0.0
        iso_ms = iso.get("acc_g1_ms") if iso else None
        iso_pts = iso.get("points_g1", avg_pts) if iso else avg_pts
        c_eff = window_of(avg_pts, args.precompute)
        nwin_g1 = FR[CURVE][2] // c_eff + 1
        mads = MADS_PER_G1_ADD[CURVE]
        traffic, traffic_src = None, None    # HBM bytes per launch of the dominant kernel: measured after the legs (measure_acc_traffic) when rocprofv3 is here, else the committed collection
        if world == 1 and args.log_m == 22 and CURVE == cg.BN254:
            for name in ("r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json"):
                try:
                    with open(os.path.join(ROOT, "profiles", name)) as f:
                        traffic = json.load(f)["dominant_kernel_traffic_bytes_per_launch"]; traffic_src = "profiles/" + name
                    break
                except Exception:
                    traffic = None
        # "state the measured stream-copy ceiling beside" the 8 TB/s peak: one 1 GiB device-to-device copy (read + write),
        # best of 5, timed with events on the stream the copy runs on (torch's current stream)
        copy_gbs = None
        if args.full:
            try:
                src = torch.empty(1 << 30, dtype=torch.uint8, device=device); dst = torch.empty_like(src)
                dst.copy_(src); torch.cuda.synchronize(device)
                best = None
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize(device)
                    t = e0.elapsed_time(e1); best = t if best is None else min(best, t)
                copy_gbs = 2.0 * (1 << 30) / (best * 1e-3) / 1e9
                del src, dst
            except Exception:                                                            # noqa: BLE001 (a side figure)
                copy_gbs = None
        free_b, total_b = torch.cuda.mem_get_info(device)
        acc_bytes = (ptb + 32.0) * iso_pts
        achieved = (acc_bytes / (iso_ms * 1e-3) / 1e9) if iso_ms else ((ptb + 32.0) * avg_pts / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0)
        cname = CURVE_NAME[CURVE]
        step_resident = {
            "value": step_value, "unit": "constraints/s", "ms_per_step": step_ms, "steps": args.steps, "warmup": args.warmup,
            "what": "the kernel pipeline of one REP3 party's prove with every input resident in HBM (masks and the peers' vectors as inputs, no PCIe, no host steps): "
                    "the figure rounds 1-3 carried as `value`",
            "step_hbm": {"algorithmic_bytes_per_step": 2048.0 * w.nc, "achieved_GBs": 2048.0 * w.nc / (elapsed / args.steps) / 1e9,
                         "frac": 2048.0 * w.nc / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS},
            "overlapped_avg_launch_ms_acc_g1": avg_ms, "overlapped_launches_acc_g1": st["msm_acc_g1_calls"], "pcie_inclusive": bool(args.pcie),
        }
        out = {
            "metric": f"Groth16 constraints/sec ({cname}, 2^{args.log_m} R1CS), one REP3 party's prove",
            "value": step_value, "unit": "constraints/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": step_ms, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "value_basis": "step_resident (inputs resident in HBM)", "rccl_ranks_seen": ranks_seen, "backend": (args.backend if dist is not None else None),
            "dtype": "u32 limbs (%d-bit modular integer arithmetic)" % FR[CURVE][2], "data": "synthetic",
            "config": {"workload": f"synthetic R1CS 2^{args.log_m} constraints-domain {cname}, REP3 co-groth16 (configs[2])",
                       "num_constraints": w.nc, "domain_size": w.m, "n_vars": w.m, "nnz": w.nnz, "share_components": 2,
                       "msm": "8 G1 + 2 G2 of ~2^%d points" % args.log_m, "msm_window": ("precomputed tables c=%s" % (args.precompute if args.precompute > 0 else "auto (20 above 3 M G1 / 1.5 M G2 points, else 17)")) if args.precompute else "c=16, per-window bucket sets", "ntt": 12, "parallelism": f"msm units (tables / table slices) over {world} rank(s): " + ",".join(f"{t}{i}/{p}->r{o}" for t, i, p, o in w.plan)},
            # frac is computed from the kernel ALONE (isolated launch, what a serial rocprofv3 trace shows); overlapped_avg_launch_ms is the same kernel
            # inside the resident step, where four streams share the CUs
            "roofline": {"bound": "hbm", "kernel": "k_msm_accumulate_pf<G1> (bucket accumulation, one launch per MSM component and table)",
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_note": ("NOT measured in this run: FETCH_SIZE + WRITE_SIZE per launch from the committed rocprofv3 --pmc collection %s (separate passes, calibrated; "
                                          "each base is gathered once per window)" % traffic_src) if traffic else "no committed counter collection for this configuration",
                         "launch_ms": iso_ms, "algorithmic_bytes_per_launch": acc_bytes, "measured_copy_ceiling_GBs": copy_gbs,
                         "overlapped_avg_launch_ms": avg_ms, "overlapped_launches": st["msm_acc_g1_calls"],
                         "note": "integer-VALU bound (v_mad_u64_u32), not HBM bound, and clocked by the chip's power management: the launch holds ~1.9 GHz "
                                 "(GRBM_GUI_ACTIVE / duration, scripts/clock_by_kernel.py) where the same additions with operands in registers hold 2.35 GHz; see DESIGN.md"},
            "roofline_g2": roof((2 * ptb + 32.0) * iso["points_g2"], iso.get("acc_g2_ms")) if iso and "acc_g2_ms" in iso else None,
            "roofline_ntt": roof(64.0 * w.m, iso["ntt_ms"], kernel="k_ntt_ct_pass x2-3 + k_bitrev_finish_lazy, one 2^%d transform (32 B read + 32 B written per element, single-pass ideal)" % args.log_m) if iso else None,
            "roofline_sort": roof((32.0 + 16.0 * nwin_g1) * iso["points_g1"], iso["sort_ms"], kernel="digit + MSD partition sort schedule of one scalar vector (32 B per scalar + 16 B per (point, window) entry)") if iso else None,
            # "MSM is integer-VALU bound; also report achieved 32-bit mul-add rate".  A launch adds every point once per window.
            # Peak = the chip-wide sustained v_mad_u64_u32 issue rate (scripts/microbench_clock.hip).
            "valu_roofline": {"kernel": "k_msm_accumulate_pf<G1>", "unit": "Tmad/s (32x32+64 multiply-adds)", "mads_per_point_addition": mads,
                              "point_additions_per_launch": iso_pts * nwin_g1,
                              "achieved": (mads * iso_pts * nwin_g1 / (iso_ms * 1e-3) / 1e12) if iso_ms else None,
                              "peak": MAD_PEAK_T, "frac": (mads * iso_pts * nwin_g1 / (iso_ms * 1e-3) / 1e12 / MAD_PEAK_T) if iso_ms else None,
                              "launch_ms": iso_ms, "note": "isolated launches; peak = sustained rate of a pure v_mad_u64_u32 loop at the 2.3 GHz it holds; the launch itself "
                                                             "holds ~1.9 GHz and issues ~570 other vector instructions (and ~390 wait states) per BN254 addition beside the multiply-adds (round 6: products by columns; ~750 before)"},
            "isolated_ms": iso,
            "stages": stage_table(iso),
            "hbm_footprint": {"device_bytes_in_use": int(total_b - free_b), "device_bytes_total": int(total_b),
                              "note": "resident while the step runs: five zkey-sized tables with their per-window precomputed copies (13 windows: 21 GB at 2^22), "
                                      "share vectors, twiddles, sort / bucket scratch of two contexts"},
            "step_resident": step_resident,
            "setup_s": {"synthetic_bases": w.setup_bases_s, "precompute_tables": w.setup_precompute_s},
        }
        if preflight is not None:
            out["preflight"] = preflight
        if world > 1:
            step_resident["what"] += "; N > 1: one process per GPU, MSM work units planned over the ranks, witness map distributed for N >= 4, one all_gather of unit results + host EC fold"
            step_resident["plan"] = ",".join(f"{t}{i}/{p}->r{o}" for t, i, p, o in w.plan)
            if multi_ent is not None:
                out["product_entry"] = multi_ent
                if "value" in multi_ent:
                    out["value"], out["ms_per_step"] = multi_ent["value"], multi_ent["ms_per_proof"]
                    out["value_basis"] = (f"product entry over {world} GPUs, the N = 1 line's basis: ONE REP3 party through cgh_session_prove_rep3_party_ex on a cgh_session_open_multi session over the job's "
                                          f"{world} devices (rank 0's process drives them, as one co-circom process would; the other ranks wait in a host-side barrier) — witness shares in host memory in, proof out, "
                                          "mask draws, mul_vec exchanges over PCIe and the host steps inside the timed call; step_resident = the per-rank resident scaling of the same proof's kernels (one process per GPU over RCCL)")
                else:
                    out["value_basis"] = "step_resident (inputs resident in HBM): the multi-device product entry FAILED on this box (product_entry.error), so this line is NOT on the N = 1 line's basis — compare with step_resident.value there"
    elif rank == 0:
        # a plain N = 1 run: the headline alone, filled in by the entry leg below
        cname = CURVE_NAME[CURVE]
        m_ = 1 << args.log_m
        out = {
            "metric": f"Groth16 constraints/sec ({cname}, 2^{args.log_m} R1CS), one REP3 party's prove",
            "value": None, "unit": "constraints/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": None, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "rccl_ranks_seen": ranks_seen, "backend": (args.backend if dist is not None else None),
            "dtype": "u32 limbs (%d-bit modular integer arithmetic)" % FR[CURVE][2], "data": "synthetic",
            "config": {"workload": f"synthetic R1CS 2^{args.log_m} constraints-domain {cname}, REP3 co-groth16 (configs[2])",
                       "num_constraints": m_ - 2, "domain_size": m_, "n_vars": m_, "nnz": 3 * (m_ - 2), "share_components": 2,
                       "msm": "8 G1 + 2 G2 of ~2^%d points" % args.log_m, "ntt": 12},
        }
    if rank == 0:
        legs = not args.no_session and world == 1

        def entry_alone(*a, **kw):
            """An entry leg with the harness's second context closed: that context belongs to the resident legs, and its idle streams would sit on
            hardware queues next to the session's own (a 2^16 party as a leg of this process: 3.8 ms with it open, 3.2 in a process that holds
            only the session, scripts/later_leg.py).  The resident legs get a new one afterwards."""
            had = w is not None and w.ctx_aux is not None
            if had:
                w.ctx_aux.sync(); w.ctx_aux.close(); w.ctx_aux = None
            try:
                return entry_leg(*a, **kw)
            finally:
                if had:
                    w.ctx_aux = cg.Context(local_rank); w.ctx_aux.set_scatter_capacity(args.scatter_cap)
        if legs:
            if w is not None:
                w.release()                                             # the session registers its own tables (another 21 GB of window copies at 2^22)
            try:
                ent = entry_alone(ctx, args.log_m, device, args.steps, args.warmup, CURVE, extras=args.full, outputs=entry_out)
                # THE HEADLINE: the reference's timed region through the product's entry
                out["value"], out["ms_per_step"] = ent["value"], ent["ms_per_proof"]
                out["value_basis"] = ("product entry: ONE REP3 party through cgh_session_prove_rep3_party_ex — witness shares in host memory in, proof out, the party's ChaCha12 mask draws, both "
                                      "mul_vec exchanges over PCIe and the O(1) host steps inside the timed call (co-circom.rs:503-506); `steps` = proofs between the two barriers. "
                                      "step_resident (--full) holds the inputs-resident kernel pipeline (the bench contract's HBM-resident figure)")
                out["product_entry"] = ent
            except Exception as e:                                      # the contract line must survive a failing leg; the failure is on the line and `value` stays the resident step
                if not resident:
                    raise                                               # no resident step to fall back on: a line without its headline is an error
                out["product_entry"] = {"error": f"{type(e).__name__}: {e}"[:400]}
        if args.dump_outputs:
            if "proof" in entry_out and "value" in out.get("product_entry", {}):
                p_ = entry_out["proof"]; q = p_.shape[0] // 8             # A (G1), B (G2), C (G1), affine
                dump_outputs(args.dump_outputs, {"proof_a": p_[:2 * q], "proof_b": p_[2 * q:6 * q], "proof_c": p_[6 * q:]})
            else:
                dump_outputs(args.dump_outputs, {"msm_" + t: v for t, v in folded.items()})
        if args.full and legs and not args.no_sizes:
            sizes = {}
            for lg in [int(x) for x in args.sizes.split(",") if x]:
                if lg == args.log_m:
                    continue
                k_ = 10 if lg <= 20 else 5
                try:
                    r_ = resident_leg(ctx, w.ctx_aux, device, lg, k_, 2, CURVE, args.precompute, args.scatter_cap)
                    e_ = entry_alone(ctx, lg, device, k_, 1, CURVE, extras=False)
                    sizes["2^%d" % lg] = {"step_resident": {k: r_[k] for k in ("ms_per_step", "value", "unit", "steps", "step_hbm")},
                                          "product_entry": {k: e_[k] for k in ("ms_per_proof", "ms_per_proof_min_inner", "ms_inner_each", "value", "unit", "proofs", "three_parties_agree", "zkey")},
                                          "roofline": r_["roofline"], "roofline_g2": r_["roofline_g2"], "roofline_ntt": r_["roofline_ntt"], "valu_roofline": r_["valu_roofline"], "isolated_ms": r_["isolated_ms"]}
                except Exception as e:                                  # noqa: BLE001
                    sizes["2^%d" % lg] = {"error": f"{type(e).__name__}: {e}"[:400]}
            out["sizes"] = sizes
            # the reference's own benchmark: Poseidon(2) Groth16 REP3 (tests/benches/poseidon_hash2.rs:175-223) = the fixture circuit, m = 256
            try:
                fxd = os.path.join(ROOT, "tests", "golden", "groth16", "bn254" if CURVE == cg.BN254 else "bls12_381", "poseidon")
                p_ = entry_alone(ctx, 0, device, 20, 3, CURVE, extras=False, files=(os.path.join(fxd, "circuit.zkey"), os.path.join(fxd, "witness.wtns")))
                out["poseidon_fixture"] = {k: p_[k] for k in ("ms_per_proof", "ms_per_proof_min_inner", "ms_inner_each", "value", "unit", "proofs", "three_parties_agree", "circuit", "entry")}
                out["poseidon_fixture"]["what"] = "one REP3 party of the reference's own bench circuit (Poseidon(2), tests/benches/poseidon_hash2.rs:175-223; 213 constraints, domain 256) through the same entry"
            except Exception as e:                                      # noqa: BLE001
                out["poseidon_fixture"] = {"error": f"{type(e).__name__}: {e}"[:400]}
            other = cg.BLS12_381 if CURVE == cg.BN254 else cg.BN254
            try:                                                        # the second curve of the reference's e2e matrix, same legs at the line's size
                r_ = resident_leg(ctx, w.ctx_aux, device, args.log_m, 5, 2, other, args.precompute, args.scatter_cap)
                e_ = entry_alone(ctx, args.log_m, device, 5, 1, other, extras=False)
                out.setdefault("session", {})[args.curve == "bn254" and "bls12_381" or "bn254"] = {
                    "curve": CURVE_NAME[other], "log_m": args.log_m,
                    "step_resident": {k: r_[k] for k in ("ms_per_step", "value", "unit", "steps", "step_hbm")},
                    "product_entry": {k: e_[k] for k in ("ms_per_proof", "ms_per_proof_min_inner", "ms_inner_each", "value", "unit", "proofs", "three_parties_agree", "zkey")},
                    "roofline": r_["roofline"], "roofline_g2": r_["roofline_g2"], "roofline_ntt": r_["roofline_ntt"], "valu_roofline": r_["valu_roofline"], "isolated_ms": r_["isolated_ms"], "stages": r_["stages"]}
            except Exception as e:                                      # noqa: BLE001
                out.setdefault("session", {})["bls12_381" if CURVE == cg.BN254 else "bn254"] = {"error": f"{type(e).__name__}: {e}"[:400]}
        if args.full and world == 1 and CURVE == cg.BN254 and not args.no_session:
            try:
                w.release()
            except Exception:                                                                # noqa: BLE001
                pass
            measured, why = measure_acc_traffic(args.log_m)
            if measured is not None:
                out["roofline"]["traffic"] = measured; out["roofline"]["traffic_note"] = why
            else:
                out["roofline"]["traffic_note"] += "; in-run measurement: " + why
        if args.full and not args.no_cpu_baseline and world == 1 and CURVE == cg.BN254:
            try:
                out["cpu_baseline"] = cpu_baseline(args.log_m)
            except Exception as e:
                out["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
        if "value" in out.get("cpu_baseline", {}):
            out["speedup_vs_cpu_baseline"] = {"step_resident": step_value / out["cpu_baseline"]["value"]}
            cb = out["cpu_baseline"]
            if "value" in cb.get("entry_twin", {}) and "value" in out.get("product_entry", {}):
                out["speedup_vs_cpu_baseline"]["value_vs_entry_twin"] = out["product_entry"]["value"] / cb["entry_twin"]["value"]
            if "ms_per_proof" in cb.get("poseidon_fixture", {}) and "ms_per_proof" in out.get("poseidon_fixture", {}):
                out["speedup_vs_cpu_baseline"]["poseidon_fixture"] = cb["poseidon_fixture"]["ms_per_proof"] / out["poseidon_fixture"]["ms_per_proof"]
            out["speedup_note"] = ("step_resident against the builder's own C++ restatement of the arkworks algorithms (kind: port), not against arkworks itself; both sides of THAT ratio exclude "
                                   "mask generation (rep3/rngs.rs:37-46: 4 x 2^22 ChaCha12 rejection-sampled draws per proof on one host thread in the reference, 0.63 s measured here, "
                                   "product_entry.ms_per_proof_host_draws), serialisation, the network rounds and zkey parsing; `value` (the product entry) includes the draws, PCIe and the host steps and has "
                                   "no CPU twin here; a reported baseline, not a measure of kernel quality (the roofline fractions are)")
        emit(out)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
