"""cogroth16-hip: MI355X (gfx950) backend for the co-groth16 prover hot path of TaceoLabs/collaborative-circom.

The product is the C-ABI shared library `libcogroth16_hip.so` (include/cogroth16_hip.h) built from csrc/ with hipcc.
This module is only a thin ctypes loader over it (directory name contains a hyphen: import it with
`importlib.import_module("collaborative-circom_amd")`).  There is NO CPU fallback: `load()` raises if the library is
missing, and `Context()` raises if no HIP device is present.
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "libcogroth16_hip.so")
HOST_LIB_PATH = os.path.join(HERE, "libcogroth16_host.so")
# planning / A-B scripts only: another build of a library (scripts/multi_device_emulation.py: the -DCG_DEBUG_KNOBS build of the host library,
# `make -C host KNOBS=1`; scripts/ntt_timing.py: a hip library built with other -D switches)
if os.environ.get("COGROTH16_HIP_LIB"):
    LIB_PATH = os.path.abspath(os.environ["COGROTH16_HIP_LIB"])
if os.environ.get("COGROTH16_HOST_LIB"):
    HOST_LIB_PATH = os.path.abspath(os.environ["COGROTH16_HOST_LIB"])

BN254, BLS12_381 = 0, 1
G1, G2 = 0, 1

_lib = None


class BackendError(RuntimeError):
    pass


def build(bls=True, jobs=8):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrc"), f"-j{jobs}", f"BLS={1 if bls else 0}"])
    if os.path.isdir(os.path.join(HERE, "host")) and os.path.exists(os.path.join(HERE, "host", "Makefile")):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "host"), f"-j{jobs}"])
    return LIB_PATH


# per-context tuning options (include/cogroth16_hip.h)
OPT_MSM_CHUNK, OPT_MSM_WINDOW, OPT_MSM_SCATTER_CAP, OPT_MSM_TABLE_ORDER, OPT_MSM_G2_SLICES, OPT_MSM_REDUCE_BATCH, OPT_MSM_ACC_SLOTS, OPT_MSM_G2_AFTER, OPT_MSM_WIDE_SMALL = 1, 2, 3, 4, 5, 6, 7, 8, 9
OPT_MSM_ONE_STREAM_LOG, OPT_MSM_OFF_MAIN_LOG, OPT_MSM_SOLO_LOG = 10, 11, 12
# process-wide options (cg_set_option)
GOPT_SUBGROUP_FULL, GOPT_COMPACT_MIN_LOG, GOPT_SORT_STAGING, GOPT_SORT_SMALL, GOPT_MSM_STAGED_OUT, GOPT_STREAM_PROBES = 1, 2, 3, 4, 5, 6
# paths of the MSM's scalar-side schedule (cg_msm_schedule_dev: 1 .. 4 can be forced, all five are reported) and the scalar fields' bit lengths
MSM_PATH_GENERAL, MSM_PATH_SMALL, MSM_PATH_PARTITION, MSM_PATH_DIRECT, MSM_PATH_PARTITION_UNSTAGED = 1, 2, 3, 4, 5
FR_BITS = {0: 254, 1: 255}
# cg_msm_stages_dev: reduction kinds, the geometry record (include/cogroth16_hip.h) and what it returns
MSM_REDUCE_SEGMENTS, MSM_REDUCE_BITSUM, MSM_REDUCE_GRID, MSM_GEOM_WORDS = 0, 1, 2, 16
MSM_MAX_PARTIALS = 512                   # classic: one per window (at most 128); bit sums: c; grid: 264 at c = 22
MsmStageGeom = collections.namedtuple("MsmStageGeom", "kind ngroups nchunks nb nsets seg_len segs group_segs bit_groups log_l log_h gc gr chunk_len slice_groups nwin")
MsmStages = collections.namedtuple("MsmStages", "geom acc_buckets acc_cont cont_state cont_bucket merged_buckets partials folded")

# every symbol include/cogroth16_hip.h declares (checked by tests/test_abi_surface.py)
ABI_SYMBOLS = [
    "cg_ctx_create", "cg_ctx_create_ex", "cg_ctx_destroy", "cg_ctx_sync", "cg_ctx_stream", "cg_ctx_set_stream", "cg_last_error", "cg_version",
    "cg_dev_alloc", "cg_dev_free", "cg_dev_free_many", "cg_dev_cache_trim", "cg_stream_group_begin", "cg_stream_group_end", "cg_dev_upload", "cg_dev_download", "cg_dev_memset_zero",
    "cg_bases_register", "cg_bases_register_device", "cg_bases_release", "cg_bases_len", "cg_bases_precompute", "cg_bases_check_on_curve", "cg_bases_check_subgroup",
    "cg_msm", "cg_msm_dev", "cg_msm_dev_begin", "cg_msm_dev_begin_multi", "cg_msm_end", "cg_msm_set_window", "cg_msm_set_chunk", "cg_ctx_set_option", "cg_ctx_get_option", "cg_set_option", "cg_get_option", "cg_msm_scalars_after", "cg_msm_set_scatter_capacity", "cg_msm_schedule_dev", "cg_msm_stages_dev",
    "cg_ntt", "cg_ntt_dev", "cg_ntt_coset_pair_dev", "cg_chacha12_fr_rand_dev", "cg_chacha12_fr_rand_dev_begin", "cg_chacha12_fr_rand_dev_finish",
    "cg_host_alloc", "cg_host_free", "cg_host_is_pinned", "cg_dev_download_begin", "cg_dev_upload_begin", "cg_stream_mark", "cg_dev_download_begin_after", "cg_copy_wait", "cg_copy_fence",
    "cg_vec_add_dev", "cg_vec_sub_dev", "cg_vec_mul_dev", "cg_vec_rep3_mul_local_dev", "cg_vec_distribute_powers_dev", "cg_vec_affine_dev", "cg_vec_fill_dev", "cg_vec_gather_strided_dev", "cg_vec_lincomb_dev", "cg_shamir_share_dev", "cg_vec_prefix_prod_dev", "cg_vec_prefix_sum_dev", "cg_vec_inverse_dev",
    "cg_spmv_csr_dev", "cg_r1cs_check_dev", "cg_qap_columns_dev", "cg_plonk_gates_count_dev", "cg_plonk_gates_emit_dev", "cg_plonk_sigma_labels_dev", "cg_vec_mul", "cg_vec_rep3_mul_local",
    "cg_plonk_additions_dev", "cg_plonk_r2_factors_dev", "cg_plonk_r3_blind_dev", "cg_plonk_r3_perm_dev", "cg_plonk_r3_gate_dev", "cg_plonk_mul4_tail_dev", "cg_plonk_r3_t_dev", "cg_plonk_r3_divide_dev",
    "cg_plonk_gate_check_dev", "cg_vec_mismatch_dev",
    "cg_point_add", "cg_point_neg", "cg_point_scalar_mul", "cg_fixed_base_create", "cg_fixed_base_mul", "cg_fixed_base_destroy", "cg_point_to_affine", "cg_point_from_affine", "cg_point_validate", "cg_fr_is_canonical", "cg_vec_check_canonical_dev", "cg_fr_op",
    "cg_fr_from_canonical", "cg_fr_to_canonical", "cg_fq_to_canonical", "cg_fq_from_canonical", "cg_point_generator",
    "cg_pairing", "cg_final_exp", "cg_fp12_mul", "cg_fp12_pow", "cg_miller_loop", "cg_pairing_check", "cg_miller_batch", "cg_miller_product", "cg_final_exp_check_batch",
    "cg_plonk_verify_scalars", "cg_plonk_verify_scalars_host", "cg_g1_lincomb_batch",
    "cg_bases_synth_multiples", "cg_bases_download", "cg_bases_from_scalars",
    "cg_dev_copy_peer", "cg_ctx_device", "cg_device_count", "cg_device_preflight",
    "cg_stats_enable", "cg_stats",
]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendError(f"{LIB_PATH} is missing: build it with `make -C collaborative-circom_amd/csrc` "
                           "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    lib.cg_last_error.restype = C.c_char_p
    lib.cg_version.restype = C.c_char_p
    lib.cg_ctx_stream.restype = C.c_void_p
    lib.cg_ctx_stream.argtypes = [C.c_void_p]
    lib.cg_bases_len.restype = C.c_size_t
    lib.cg_bases_len.argtypes = [C.c_void_p]
    _lib = lib
    return lib


def _chk(rc):
    if rc != 0:
        raise BackendError(f"cogroth16_hip error {rc}: {load().cg_last_error().decode()}")


def _hp(a):
    """host pointer of a numpy array (or None)"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dp(x):
    """device pointer: DevBuf, int, torch tensor (data_ptr) or None"""
    if x is None:
        return None
    if isinstance(x, DevBuf):
        return C.c_void_p(x.ptr)
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    raise TypeError(f"not a device pointer: {type(x)}")


def _fa(a):
    """contiguous uint64 array of host-side field constants (or None)"""
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint64)


def _ptr_list(bufs):
    """array of device pointers (or None); a None entry is NULL"""
    if bufs is None:
        return None
    return (C.c_void_p * max(1, len(bufs)))(*[None if b is None else _dp(b).value for b in bufs])


def _share_table(bufs, nv):
    """pointer table [v * 2 + j] of nv vectors from the flat list of nv x k buffers [a0, (a1), b0, (b1), ..]: NULL second entries for k == 1"""
    if bufs is None:
        return None
    per = len(bufs) // nv
    assert per in (1, 2) and per * nv == len(bufs), f"{len(bufs)} buffers are not 1 or 2 components of {nv} vectors"
    tab = (C.c_void_p * (2 * nv))()
    for v in range(nv):
        for j in range(per):
            b = bufs[v * per + j]
            tab[2 * v + j] = None if b is None else _dp(b).value
    return tab


def fq_limbs(curve):
    return 6 if curve == BLS12_381 else 4


def point_words(curve, group, coords):
    return fq_limbs(curve) * (1 if group == G1 else 2) * coords


class DevBuf:
    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = C.c_void_p()
        _chk(load().cg_dev_alloc(ctx.h, C.c_size_t(nbytes), C.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _chk(load().cg_dev_upload(self.ctx.h, C.c_void_p(self.ptr), _hp(arr), C.c_size_t(arr.nbytes)))
        return self

    def download(self, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        _chk(load().cg_dev_download(self.ctx.h, _hp(out), C.c_void_p(self.ptr), C.c_size_t(out.nbytes)))
        return out

    def zero(self):
        _chk(load().cg_dev_memset_zero(self.ctx.h, C.c_void_p(self.ptr), C.c_size_t(self.nbytes)))
        return self

    def free(self):
        if self.ptr:
            _chk(load().cg_dev_free(self.ctx.h, C.c_void_p(self.ptr)))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Bases:
    def __init__(self, ctx, curve, group, handle, n):
        self.ctx, self.curve, self.group, self.h, self.n = ctx, curve, group, handle, n

    def release(self):
        if self.h:
            load().cg_bases_release(self.h)
            self.h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Context:
    """One per MPC party thread (mirrors `&mut self` of the reference drivers)."""

    CHAIN, BULK = 1, 2          # cg_ctx_create_ex flags: the context of a dependency chain / the context that fills the chip next to it

    def __init__(self, device=0, flags=0):
        h = C.c_void_p()
        _chk(load().cg_ctx_create_ex(int(device), C.c_uint32(int(flags)), C.byref(h)))
        self.h = h
        self.device = device

    def set_option(self, option, value):
        """per-context tuning table (include/cogroth16_hip.h: CG_OPT_*); never changes results"""
        _chk(load().cg_ctx_set_option(self.h, int(option), C.c_int64(int(value))))

    def get_option(self, option):
        v = C.c_int64(0)
        _chk(load().cg_ctx_get_option(self.h, int(option), C.byref(v)))
        return int(v.value)

    def msm_set_chunk(self, entries):
        """entries per accumulation lane for this context's MSMs (0 = automatic): short-lived workgroups next to a latency chain"""
        _chk(load().cg_msm_set_chunk(self.h, C.c_uint32(int(entries))))

    def close(self):
        if self.h:
            load().cg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _chk(load().cg_ctx_sync(self.h))

    @property
    def stream(self):
        return load().cg_ctx_stream(self.h)

    def set_stream(self, hip_stream):
        """launch on a stream owned by the host application (e.g. torch.cuda.Stream().cuda_stream)"""
        _chk(load().cg_ctx_set_stream(self.h, C.c_void_p(int(hip_stream))))

    # ---- memory
    def free_many(self, bufs):
        """several DevBufs released behind ONE release mark (cg_dev_free_many)"""
        live = [b for b in bufs if b.ptr]
        arr = (C.c_void_p * max(1, len(live)))(*[b.ptr for b in live])
        _chk(load().cg_dev_free_many(self.h, arr, C.c_size_t(len(live))))
        for b in live: b.ptr = 0

    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DevBuf(self, max(arr.nbytes, 16)).upload(arr)

    # ---- Rep3Rand's O(n) draws on the device (cg_chacha12_fr_rand_dev)
    def chacha12_fr_rand(self, curve, seed, word_pos, n):
        """n x F::rand over ChaCha12Rng::from_seed(seed) positioned at word_pos: (DevBuf of n x 32 B, word position afterwards)"""
        buf = self.alloc(max(n * 32, 16)); after = C.c_uint64(0)
        _chk(load().cg_chacha12_fr_rand_dev(self.h, curve, bytes(seed), C.c_uint64(word_pos), C.c_size_t(n), C.c_void_p(buf.ptr), C.byref(after)))
        return buf, after.value

    def chacha12_fr_rand_begin(self, curve, seed, word_pos, n):
        """the same draws enqueued and not waited for: (DevBuf, ticket for chacha12_fr_rand_finish)"""
        buf = self.alloc(max(n * 32, 16)); tk = C.c_int32(-1)
        _chk(load().cg_chacha12_fr_rand_dev_begin(self.h, curve, bytes(seed), C.c_uint64(word_pos), C.c_size_t(n), C.c_void_p(buf.ptr), C.byref(tk)))
        return buf, tk.value

    def chacha12_fr_rand_finish(self, ticket):
        """waits for the draw of that ticket: word position afterwards"""
        after = C.c_uint64(0)
        _chk(load().cg_chacha12_fr_rand_dev_finish(self.h, C.c_int32(ticket), C.byref(after)))
        return after.value

    # ---- page-locked staging + asynchronous copies (exchange chunks move under the compute)
    def host_alloc(self, shape, dtype=np.uint64):
        """page-locked numpy array (free with host_free)"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        _chk(load().cg_host_alloc(C.c_size_t(n), C.byref(p)))
        arr = np.ctypeslib.as_array((C.c_uint8 * max(n, 1)).from_address(p.value))[:n].view(dtype).reshape(shape)
        return arr

    def host_free(self, arr): _chk(load().cg_host_free(C.c_void_p(arr.ctypes.data)))

    def download_begin(self, h_dst, d_src, nbytes=None, offset=0):
        t = C.c_int32(-1)
        _chk(load().cg_dev_download_begin(self.h, _hp(h_dst), C.c_void_p(_dp(d_src).value + offset), C.c_size_t(h_dst.nbytes if nbytes is None else nbytes), C.byref(t)))
        return t.value

    def stream_mark(self):
        """a point of the context's stream order (everything enqueued so far) that later downloads can be ordered behind"""
        m = C.c_int32(-1)
        _chk(load().cg_stream_mark(self.h, C.byref(m)))
        return int(m.value)

    def download_begin_after(self, h_dst, d_src, mark, nbytes=None, offset=0):
        """like download_begin, ordered behind `mark` instead of behind everything the stream holds now"""
        t = C.c_int32(-1)
        nb = h_dst.nbytes if nbytes is None else nbytes
        _chk(load().cg_dev_download_begin_after(self.h, C.c_void_p(h_dst.ctypes.data), C.c_void_p(_dp(d_src).value + offset), C.c_size_t(nb), int(mark), C.byref(t)))
        return int(t.value)

    def upload_begin(self, d_dst, h_src, after_stream=True, nbytes=None, offset=0):
        t = C.c_int32(-1)
        _chk(load().cg_dev_upload_begin(self.h, C.c_void_p(_dp(d_dst).value + offset), _hp(h_src), C.c_size_t(h_src.nbytes if nbytes is None else nbytes), int(bool(after_stream)), C.byref(t)))
        return t.value

    def copy_wait(self, ticket): _chk(load().cg_copy_wait(self.h, int(ticket)))
    def copy_fence(self, ticket): _chk(load().cg_copy_fence(self.h, int(ticket)))

    # ---- pairing batches (cg_miller_batch / cg_miller_product / cg_final_exp_check_batch): one lane per (P, Q) pair
    def miller_batch(self, curve, g1, g2):
        """the n Miller values of packed affine pairs (g1[i], g2[i]) as (n, 2, 3, 2, limbs); cg.final_exp of one is the pairing"""
        g1, g2 = _pairs(curve, g1, g2)
        out = np.zeros((g1.shape[0], 2, 3, 2, fq_limbs(curve)), dtype=np.uint64)
        _chk(load().cg_miller_batch(self.h, curve, _hp(g1), _hp(g2), C.c_size_t(g1.shape[0]), _hp(out)))
        return out

    def miller_product(self, curve, g1, g2, scalars128=None):
        """product of the Miller values of (k_i g1[i], g2[i]), no final exponentiation; scalars128: (n, 2) u64 canonical 128-bit integers k_i"""
        g1, g2 = _pairs(curve, g1, g2)
        k = None if scalars128 is None else np.ascontiguousarray(scalars128, dtype=np.uint64).reshape(g1.shape[0], 2)
        out = np.zeros((2, 3, 2, fq_limbs(curve)), dtype=np.uint64)
        _chk(load().cg_miller_product(self.h, curve, _hp(g1), _hp(g2), _hp(k), C.c_size_t(g1.shape[0]), _hp(out)))
        return out

    def final_exp_check_batch(self, curve, values, k, target):
        """flags[i] = FE(values[i k] * .. * values[i k + k - 1]) == target for n groups of k Miller values"""
        nq = fq_limbs(curve)
        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 12 * nq)
        n = v.shape[0] // int(k)
        assert n * int(k) == v.shape[0]
        ok = np.zeros(n, dtype=np.int32)
        _chk(load().cg_final_exp_check_batch(self.h, curve, _hp(v), int(k), C.c_size_t(n), _hp(np.ascontiguousarray(target, dtype=np.uint64)), _hp(ok)))
        return ok.astype(bool)

    # ---- MSM
    def plonk_verify_scalars(self, curve, key, commits, evals, pubs, coeff128=None):
        """cg_plonk_verify_scalars: one GPU lane per proof; see plonk_verify_scalars_host for the arguments and the result"""
        return _plonk_verify_scalars(self.h, curve, key, commits, evals, pubs, coeff128)

    def g1_lincomb_batch(self, curve, points, scalars):
        """out[g] = sum_k scalars[g, k] points[g, k]: points (groups, K, point words) packed affine G1, scalars (groups, K, 4) Montgomery"""
        nq = fq_limbs(curve)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64); groups, k = scalars.shape[0], scalars.shape[1]
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(groups, k, 2 * nq)
        out = np.zeros((groups, 2 * nq), dtype=np.uint64)
        _chk(load().cg_g1_lincomb_batch(self.h, curve, _hp(points), _hp(scalars), C.c_size_t(groups), int(k), _hp(out)))
        return out

    def register_bases(self, curve, group, points, stride=None, infinity_offset=-1):
        pts = np.ascontiguousarray(points)
        rec = point_words(curve, group, 2) * 8
        stride = stride or rec
        n = pts.nbytes // stride
        h = C.c_void_p()
        _chk(load().cg_bases_register(self.h, curve, group, _hp(pts), C.c_size_t(n), C.c_size_t(stride), C.c_int64(infinity_offset), C.byref(h)))
        return Bases(self, curve, group, h, n)

    def register_bases_device(self, curve, group, d_points, n):
        h = C.c_void_p()
        _chk(load().cg_bases_register_device(self.h, curve, group, _dp(d_points), C.c_size_t(n), C.byref(h)))
        return Bases(self, curve, group, h, n)

    def check_on_curve(self, bases):
        """(number of non-infinity points off the curve, index of the first one or None) — device-side zkey validation"""
        nb, fb = C.c_uint64(0), C.c_uint64(0)
        _chk(load().cg_bases_check_on_curve(self.h, bases.h, C.byref(nb), C.byref(fb)))
        return nb.value, (None if fb.value == 2**64 - 1 else fb.value)

    def check_subgroup(self, bases):
        """(number of non-infinity points outside the prime-order subgroup, index of the first one or None); assumes on-curve points"""
        nb, fb = C.c_uint64(0), C.c_uint64(0)
        _chk(load().cg_bases_check_subgroup(self.h, bases.h, C.byref(nb), C.byref(fb)))
        return nb.value, (None if fb.value == 2**64 - 1 else fb.value)

    def precompute_bases(self, bases, c=20):
        """per-window precomputed tables (one-time, (254/c + 1) x memory): fewer mixed additions per point afterwards"""
        _chk(load().cg_bases_precompute(self.h, bases.h, int(c)))

    def synth_bases(self, curve, group, first, n):
        """device-side table [(first+i)*G] (bench / test tooling)"""
        h = C.c_void_p()
        _chk(load().cg_bases_synth_multiples(self.h, curve, group, C.c_uint64(first), C.c_size_t(n), C.byref(h)))
        return Bases(self, curve, group, h, n)

    def bases_from_scalars(self, curve, group, d_scalars, n):
        """device-side table [s_i * G] for n device-resident Montgomery scalars (setup tooling: synthetic CRS)"""
        h = C.c_void_p()
        _chk(load().cg_bases_from_scalars(self.h, curve, group, _dp(d_scalars), C.c_size_t(n), C.byref(h)))
        return Bases(self, curve, group, h, n)

    def bases_download(self, bases, offset, n):
        out = np.zeros((n, point_words(bases.curve, bases.group, 2)), dtype=np.uint64)
        _chk(load().cg_bases_download(self.h, bases.h, C.c_size_t(offset), C.c_size_t(n), _hp(out)))
        return out

    def msm(self, bases, scalars, offset=0, n=None):
        """host scalars: list of k arrays (n,4) uint64 -> (k, 3*coord_words) Jacobian"""
        sc = [np.ascontiguousarray(s, dtype=np.uint64) for s in scalars]
        n = sc[0].size // 4 if n is None else n
        k = len(sc)
        out = np.zeros((k, point_words(bases.curve, bases.group, 3)), dtype=np.uint64)
        ptrs = (C.c_void_p * k)(*[s.ctypes.data for s in sc])
        _chk(load().cg_msm(self.h, bases.h, C.c_size_t(offset), C.c_size_t(n), ptrs, k, _hp(out)))
        return out

    def msm_dev(self, bases, d_scalars, n, offset=0):
        k = len(d_scalars)
        out = np.zeros((k, point_words(bases.curve, bases.group, 3)), dtype=np.uint64)
        ptrs = (C.c_void_p * k)(*[_dp(s).value for s in d_scalars])
        _chk(load().cg_msm_dev(self.h, bases.h, C.c_size_t(offset), C.c_size_t(n), ptrs, k, _hp(out)))
        return out

    def msm_dev_begin(self, bases, d_scalars, n, offset=0):
        k = len(d_scalars)
        ptrs = (C.c_void_p * k)(*[_dp(s).value for s in d_scalars])
        t = C.c_int32(-1)
        _chk(load().cg_msm_dev_begin(self.h, bases.h, C.c_size_t(offset), C.c_size_t(n), ptrs, k, C.byref(t)))
        return (t.value, k, bases.curve, bases.group)

    def msm_dev_begin_multi(self, bases_list, d_scalars, n, offsets=None):
        """several tables x the same scalar vectors: one digit/sort schedule per vector shared by all tables"""
        nb, k = len(bases_list), len(d_scalars)
        tabs = (C.c_void_p * nb)(*[b.h.value for b in bases_list])
        offs = (C.c_size_t * nb)(*([0] * nb if offsets is None else offsets))
        ptrs = (C.c_void_p * k)(*[_dp(s).value for s in d_scalars])
        tk = (C.c_int32 * nb)()
        _chk(load().cg_msm_dev_begin_multi(self.h, nb, tabs, offs, C.c_size_t(n), ptrs, k, tk))
        return [(tk[i], k, bases_list[i].curve, bases_list[i].group) for i in range(nb)]

    def msm_end(self, ticket):
        t, k, curve, group = ticket
        out = np.zeros((k, point_words(curve, group, 3)), dtype=np.uint64)
        _chk(load().cg_msm_end(self.h, t, _hp(out)))
        return out

    def set_scatter_capacity(self, cap):
        """0 = automatic optimistic capacity, > 0 forced (tests), < 0 always the exact two-pass sort"""
        _chk(load().cg_msm_set_scatter_capacity(self.h, int(cap)))

    def set_msm_window(self, c):
        _chk(load().cg_msm_set_window(self.h, int(c)))

    def msm_schedule(self, curve, d_scalars, n, c, shared=False, path=0, cap=0, out=None):
        """the scalar-side schedule of one device scalar vector (cg_msm_schedule_dev) -> (counts, offsets, sorted, path_taken, overflow);
        path: 0 = what an MSM call selects, MSM_PATH_* = forced; out: (counts, offsets, sorted) uint32 arrays to fill instead of new ones"""
        nwin = FR_BITS[curve] // int(c) + 1
        nbuckets = (1 if shared else nwin) << max(int(c) - 1, 0)
        if out is None:
            out = (np.empty(nbuckets, dtype=np.uint32), np.empty(nbuckets, dtype=np.uint32), np.empty(nbuckets * int(cap) if path == MSM_PATH_DIRECT else nwin * int(n), dtype=np.uint32))
        counts, offsets, sorted_ = out
        taken, overflow = C.c_int32(0), C.c_uint32(0)
        _chk(load().cg_msm_schedule_dev(self.h, int(curve), _dp(d_scalars), C.c_size_t(n), int(c), int(bool(shared)), int(path), C.c_uint32(cap), _hp(counts), _hp(offsets), _hp(sorted_),
                                        C.byref(taken), C.byref(overflow)))
        return counts, offsets, sorted_, taken.value, overflow.value

    def msm_stages(self, bases, c, entries, chunk_len, schedules, cap=0, want=("acc", "merged", "partials", "folded"), out=None):
        """the point side of the MSM stage by stage (cg_msm_stages_dev) over `schedules` = [(counts, offsets, sorted)] of uint32 host arrays, one
        per set -> MsmStages.  want: which stages come down ("acc" = buckets, continuation pieces with states and tags after the accumulation;
        "merged" = buckets after the merges; "partials"; "folded").  out: a dict of arrays to fill instead of new ones (tests of refusals)."""
        nsets = len(schedules)
        nwin = FR_BITS[bases.curve] // int(c) + 1
        scheds = [tuple(np.ascontiguousarray(a, dtype=np.uint32) for a in s) for s in schedules]
        nbuckets = scheds[0][0].size
        nchunks = max(1, -(-int(entries) // max(int(chunk_len), 1)))
        aw, jw = point_words(bases.curve, bases.group, 2), point_words(bases.curve, bases.group, 3)
        geom = np.zeros(MSM_GEOM_WORDS, dtype=np.uint32)
        o = dict(out or {})
        if "acc" in want:
            o.setdefault("acc_buckets", np.empty((nsets, nbuckets, aw), dtype=np.uint64)); o.setdefault("acc_cont", np.empty((nsets, nchunks, aw), dtype=np.uint64))
            o.setdefault("cont_state", np.empty((nsets, nchunks), dtype=np.uint32)); o.setdefault("cont_bucket", np.empty((nsets, nchunks), dtype=np.uint32))
        if "merged" in want:
            o.setdefault("merged_buckets", np.empty((nsets, nbuckets, aw), dtype=np.uint64))
        if "partials" in want:                             # how many there are per set comes back in the geometry record: room for the most any window gives
            o.setdefault("partials", np.empty(nsets * MSM_MAX_PARTIALS * jw, dtype=np.uint64))
        if "folded" in want:
            o.setdefault("folded", np.empty((nsets, jw), dtype=np.uint64))
        ptrs = [(C.c_void_p * nsets)(*[s[k].ctypes.data for s in scheds]) for k in range(3)]
        _chk(load().cg_msm_stages_dev(self.h, bases.h, int(c), C.c_size_t(int(entries)), C.c_uint32(int(chunk_len)), C.c_uint32(int(cap)), nsets, ptrs[0], ptrs[1], ptrs[2],
                                      _hp(o.get("acc_buckets")), _hp(o.get("acc_cont")), _hp(o.get("cont_state")), _hp(o.get("cont_bucket")), _hp(o.get("merged_buckets")),
                                      _hp(o.get("partials")), _hp(o.get("folded")), _hp(geom)))
        g = MsmStageGeom(*[int(v) for v in geom])
        assert g.nchunks == nchunks and g.nwin == nwin and g.ngroups <= MSM_MAX_PARTIALS, g
        if o.get("partials") is not None and o["partials"].ndim == 1:
            o["partials"] = o["partials"][:nsets * g.ngroups * jw].reshape(nsets, g.ngroups, jw)
        return MsmStages(geom=g, **{k: o.get(k) for k in MsmStages._fields if k != "geom"})

    # ---- NTT
    def ntt(self, curve, vecs, group_gen, inverse=False, coset_gen=None):
        """host vectors (list of (n,4) arrays), transformed copies are returned"""
        out = [np.ascontiguousarray(v, dtype=np.uint64).copy() for v in vecs]
        k = len(out)
        n = out[0].size // 4
        ptrs = (C.c_void_p * k)(*[v.ctypes.data for v in out])
        gg = np.ascontiguousarray(group_gen, dtype=np.uint64)
        cg = None if coset_gen is None else np.ascontiguousarray(coset_gen, dtype=np.uint64)
        _chk(load().cg_ntt(self.h, curve, ptrs, k, C.c_size_t(n), _hp(gg), int(inverse), _hp(cg)))
        return out

    def ntt_dev(self, curve, d_vecs, n, group_gen, inverse=False, coset_gen=None):
        k = len(d_vecs)
        ptrs = (C.c_void_p * k)(*[_dp(v).value for v in d_vecs])
        gg = np.ascontiguousarray(group_gen, dtype=np.uint64)
        cg = None if coset_gen is None else np.ascontiguousarray(coset_gen, dtype=np.uint64)
        _chk(load().cg_ntt_dev(self.h, curve, ptrs, k, C.c_size_t(n), _hp(gg), int(inverse), _hp(cg)))

    def ntt_coset_pair_dev(self, curve, d_vecs, n, group_gen, coset_gen):
        """v <- NTT(g^i * iNTT(v)_i) in one call (groth16.rs:175-188), natural order in and out"""
        k = len(d_vecs)
        ptrs = (C.c_void_p * k)(*[_dp(v).value for v in d_vecs])
        _chk(load().cg_ntt_coset_pair_dev(self.h, curve, ptrs, k, C.c_size_t(n), _hp(np.ascontiguousarray(group_gen, dtype=np.uint64)), _hp(np.ascontiguousarray(coset_gen, dtype=np.uint64))))

    # ---- vector ops (device operands)
    def vec_add(self, curve, out, a, b, n): _chk(load().cg_vec_add_dev(self.h, curve, _dp(out), _dp(a), _dp(b), C.c_size_t(n)))
    def vec_sub(self, curve, out, a, b, n): _chk(load().cg_vec_sub_dev(self.h, curve, _dp(out), _dp(a), _dp(b), C.c_size_t(n)))
    def vec_mul(self, curve, out, a, b, n): _chk(load().cg_vec_mul_dev(self.h, curve, _dp(out), _dp(a), _dp(b), C.c_size_t(n)))

    def vec_rep3_mul_local(self, curve, out, aa, ab, ba, bb, mask, n):
        _chk(load().cg_vec_rep3_mul_local_dev(self.h, curve, _dp(out), _dp(aa), _dp(ab), _dp(ba), _dp(bb), _dp(mask), C.c_size_t(n)))

    def vec_distribute_powers(self, curve, v, n, g, c):
        _chk(load().cg_vec_distribute_powers_dev(self.h, curve, _dp(v), C.c_size_t(n), _hp(np.ascontiguousarray(g, dtype=np.uint64)), _hp(np.ascontiguousarray(c, dtype=np.uint64))))

    def vec_affine(self, curve, out, a, n, c, d=None):
        _chk(load().cg_vec_affine_dev(self.h, curve, _dp(out), _dp(a), C.c_size_t(n), _hp(np.ascontiguousarray(c, dtype=np.uint64)),
                                      _hp(None if d is None else np.ascontiguousarray(d, dtype=np.uint64))))

    def vec_fill(self, curve, v, n, value): _chk(load().cg_vec_fill_dev(self.h, curve, _dp(v), C.c_size_t(n), _hp(np.ascontiguousarray(value, dtype=np.uint64))))
    def vec_gather_strided(self, curve, out, src, n, offset, stride): _chk(load().cg_vec_gather_strided_dev(self.h, curve, _dp(out), _dp(src), C.c_size_t(n), C.c_size_t(offset), C.c_size_t(stride)))
    def vec_lincomb(self, curve, out, out_off, out_stride, n, srcs, src_off, src_stride, coeffs):
        """out[out_off + i*out_stride] = sum_j coeffs[j] * srcs[j][src_off[j] + i*src_stride[j]] (element units, negative strides allowed)"""
        k = len(srcs)
        ptrs = (C.c_void_p * k)(*[_dp(x).value for x in srcs])
        offs = (C.c_int64 * k)(*[int(x) for x in src_off]); strides = (C.c_int64 * k)(*[int(x) for x in src_stride])
        _chk(load().cg_vec_lincomb_dev(self.h, curve, _dp(out), C.c_int64(out_off), C.c_int64(out_stride), C.c_size_t(n), k, ptrs, offs, strides,
                                       _hp(np.ascontiguousarray(coeffs, dtype=np.uint64))))

    def shamir_share(self, curve, secrets, coeffs, coeff_off, coeff_stride, n, degree, outs, out_off=0, out_stride=1):
        """outs[p][out_off + i*out_stride] = secrets[i] + sum_{j=1..degree} coeffs[coeff_off + i*coeff_stride + j - 1] * (p + 1)^j, all parties in one launch"""
        ptrs = (C.c_void_p * len(outs))(*[_dp(x).value for x in outs])
        _chk(load().cg_shamir_share_dev(self.h, curve, _dp(secrets), _dp(coeffs), C.c_int64(coeff_off), C.c_int64(coeff_stride), C.c_size_t(n), int(degree),
                                        len(outs), ptrs, C.c_int64(out_off), C.c_int64(out_stride)))

    # ---- co-plonk's fused kernels (csrc/plonk_kernels.hpp).  A share table is a flat list of nv x k buffers [a0, (a1), b0, (b1), ..]; it
    # becomes the ABI's pointer table [v * 2 + j] with NULL second entries for k == 1.  None (a table, an entry, a constant) is passed as NULL.
    def plonk_additions(self, curve, order, n, ids, coeffs, pub, n_inputs, public_component, ext_a, ext_b, n_priv, order_off=0):
        """one dependency level of round 1's additions (cg_plonk_additions_dev): the n additions order[order_off ..] of the list (ids, coeffs),
        written to ext[n_priv + a] of every component; ext_b = None for one share component"""
        po = None if order is None else C.c_void_p(_dp(order).value + 4 * int(order_off))
        _chk(load().cg_plonk_additions_dev(self.h, curve, po, C.c_size_t(n), _dp(ids), _dp(coeffs), _dp(pub), C.c_uint32(n_inputs), int(public_component),
                                           _dp(ext_a), _dp(ext_b), C.c_size_t(n_priv)))

    def plonk_r2_factors(self, curve, k, public_component, n, pw, pw_stride, sigmas, sigma_stride, coeffs, wires, outs):
        """round 2's six factors (cg_plonk_r2_factors_dev): wires = 3 x k buffers [a0, a1, b0, ..], outs = 6 x k likewise; coeffs = beta, beta k1, beta k2, gamma"""
        _chk(load().cg_plonk_r2_factors_dev(self.h, curve, int(k), int(public_component), C.c_size_t(n), _dp(pw), C.c_size_t(pw_stride), _ptr_list(sigmas), C.c_size_t(sigma_stride),
                                            _hp(_fa(coeffs)), _share_table(wires, 3), _share_table(outs, 6)))

    def plonk_r3_blind(self, curve, k, n, pw, omega, blind, outs):
        """round 3's blinding polynomials on pw (cg_plonk_r3_blind_dev): blind = k x 9 coefficients b_1..b_9 per component, outs = 5 x k buffers ap, bp, cp, zp, zwp"""
        _chk(load().cg_plonk_r3_blind_dev(self.h, curve, int(k), C.c_size_t(n), _dp(pw), _hp(_fa(omega)), _hp(_fa(blind)), _share_table(outs, 5)))

    def plonk_r3_perm(self, curve, k, public_component, n, pw, sigmas, coeffs, wires, outs):
        """round 3's six permutation factors (cg_plonk_r3_perm_dev): the arguments of plonk_r2_factors without the strides"""
        _chk(load().cg_plonk_r3_perm_dev(self.h, curve, int(k), int(public_component), C.c_size_t(n), _dp(pw), _ptr_list(sigmas), _hp(_fa(coeffs)),
                                         _share_table(wires, 3), _share_table(outs, 6)))

    def plonk_r3_gate(self, curve, k, public_component, n, q, lagrange, n_lagrange, ins, z1, outs):
        """the gate constraint and its blinding twin (cg_plonk_r3_gate_dev): q = qm, ql, qr, qo, qc; lagrange = n_lagrange rows of n; ins = 11 x k buffers
        buffer_a, a b, a b', a' b, a' b', a, b, c, a', b', c'; z1 = 4 constants; outs = 2 x k buffers e1, e1z"""
        _chk(load().cg_plonk_r3_gate_dev(self.h, curve, int(k), int(public_component), C.c_size_t(n), _ptr_list(q), _dp(lagrange), C.c_size_t(n_lagrange),
                                         _share_table(ins, 11), _hp(_fa(z1)), _share_table(outs, 2)))

    def plonk_mul4_tail(self, curve, k, n, prods, z, rz):
        """the linear end of mul4vec_post (cg_plonk_mul4_tail_dev): prods = 8 x k buffers, z = 3 x 4 constants Z1, Z2, Z3, rz = k buffers"""
        _chk(load().cg_plonk_mul4_tail_dev(self.h, curve, int(k), C.c_size_t(n), _share_table(prods, 8), _hp(_fa(z)), _share_table(rz, 1)))

    def plonk_r3_t(self, curve, k, public_component, n, l1, ins, alpha, outs):
        """t and tz before the inverse NTTs (cg_plonk_r3_t_dev): ins = 8 x k buffers e1, e1z, e2, e3, e2z, e3z, z, z'; outs = 2 x k buffers t, tz"""
        _chk(load().cg_plonk_r3_t_dev(self.h, curve, int(k), int(public_component), C.c_size_t(n), _dp(l1), _share_table(ins, 8), _hp(_fa(alpha)), _share_table(outs, 2)))

    def plonk_r3_divide(self, curve, k, n, t, tz):
        """the division by X^n - 1 and + tz, in place on t (cg_plonk_r3_divide_dev): t, tz = k buffers of 4n elements"""
        _chk(load().cg_plonk_r3_divide_dev(self.h, curve, int(k), C.c_size_t(n), _share_table(t, 1), _share_table(tz, 1)))

    def vec_prefix_prod(self, curve, out, src, n): _chk(load().cg_vec_prefix_prod_dev(self.h, curve, _dp(out), _dp(src), C.c_size_t(n)))
    def vec_prefix_sum(self, curve, out, src, n): _chk(load().cg_vec_prefix_sum_dev(self.h, curve, _dp(out), _dp(src), C.c_size_t(n)))
    def vec_inverse(self, curve, out, src, n): _chk(load().cg_vec_inverse_dev(self.h, curve, _dp(out), _dp(src), C.c_size_t(n)))

    def vec_check_canonical(self, curve, d_vec, n, d_count):
        """cg_vec_check_canonical_dev: ADDS the number of the n elements of d_vec whose limbs are not below the modulus to the u64 in the 8-byte
        device buffer d_count (the caller zeroes it); enqueued on the context's stream"""
        _chk(load().cg_vec_check_canonical_dev(self.h, curve, _dp(d_vec), C.c_size_t(n), _dp(d_count)))

    def r1cs_check(self, curve, mats, n_rows, witness, result, nnz_total=0, form=0):
        """cg_r1cs_check_dev: mats = three (row_ptr, col, coeff) device triples (A, B, C); result = 16-byte device buffer (count, first failing row);
        form 0 = chosen by size, 1 = a lane per row triple, 2 = a wave per row triple"""
        _chk(load().cg_r1cs_check_dev(self.h, curve, _ptr_list([m[0] for m in mats]), _ptr_list([m[1] for m in mats]), _ptr_list([m[2] for m in mats]),
                                      C.c_size_t(n_rows), C.c_size_t(nnz_total), int(form), _dp(witness), _dp(result)))

    def qap_columns(self, curve, col_ptr, row, coeff, n_cols, lagrange, out, long_min=0):
        """cg_qap_columns_dev: out[i] = sum over the entries of column i of coeff * lagrange[row] (column-major matrix); long_min = entries from
        which the workgroup, not one lane, sums a column (0 = the library's default)"""
        _chk(load().cg_qap_columns_dev(self.h, curve, _dp(col_ptr), _dp(row), _dp(coeff), C.c_size_t(n_cols), C.c_uint32(long_min), _dp(lagrange), _dp(out)))

    def plonk_gates_count(self, curve, mats, n_rows, nnz_total, counts, offsets):
        """cg_plonk_gates_count_dev: mats = three canonical (row_ptr, col, coeff) device triples (wires ascending, merged, no zero coefficient);
        counts / offsets = device buffers of n_rows + 1 u32 (additions per row, their exclusive scan); returns the additions of the circuit"""
        total = C.c_size_t(0)
        _chk(load().cg_plonk_gates_count_dev(self.h, curve, _ptr_list([m[0] for m in mats]), _ptr_list([m[1] for m in mats]), _ptr_list([m[2] for m in mats]),
                                             C.c_size_t(n_rows), C.c_size_t(nnz_total), _dp(counts), _dp(offsets), C.byref(total)))
        return int(total.value)

    def plonk_gates_emit(self, curve, mats, n_rows, n_wires, n_public, counts, offsets, n_additions, domain_size, maps, q, add_ids, add_f):
        """cg_plonk_gates_emit_dev: maps = 3 device buffers of n_public + n_rows + n_additions u32, q = 5 device vectors of domain_size elements
        (qm, ql, qr, qo, qc), add_ids / add_f = 2 u32 / 2 elements per addition"""
        _chk(load().cg_plonk_gates_emit_dev(self.h, curve, _ptr_list([m[0] for m in mats]), _ptr_list([m[1] for m in mats]), _ptr_list([m[2] for m in mats]),
                                            C.c_size_t(n_rows), C.c_size_t(n_wires), C.c_size_t(n_public), _dp(counts), _dp(offsets), C.c_size_t(n_additions),
                                            C.c_size_t(domain_size), _ptr_list(maps), _ptr_list(q), _dp(add_ids), _dp(add_f)))

    def plonk_sigma_labels(self, curve, prev, omega_powers, domain_size, k1, k2, sigma):
        """cg_plonk_sigma_labels_dev: sigma[p] = k_(prev[p] / n) * omega_powers[prev[p] % n] for p < 3n"""
        _chk(load().cg_plonk_sigma_labels_dev(self.h, curve, _dp(prev), _dp(omega_powers), C.c_size_t(domain_size), _hp(np.ascontiguousarray(k1, dtype=np.uint64)),
                                              _hp(np.ascontiguousarray(k2, dtype=np.uint64)), _dp(sigma)))

    def plonk_gate_check(self, curve, maps, n_constraints, q, q_stride, domain_size, pub, n_public, ext, n_wires, result):
        """cg_plonk_gate_check_dev: maps = 3 device buffers of n_constraints u32 (a, b, c), q = 5 device vectors (qm, ql, qr, qo, qc) read at
        i * q_stride, pub = n_public + 1 elements (entry 0 zero), ext = the extended witness of the wires beyond them; result = 16-byte device
        buffer (count, first failing row)"""
        _chk(load().cg_plonk_gate_check_dev(self.h, curve, _ptr_list(maps), C.c_size_t(n_constraints), _ptr_list(q), C.c_size_t(q_stride), C.c_size_t(domain_size),
                                            _dp(pub), C.c_uint32(n_public), _dp(ext), C.c_size_t(n_wires), _dp(result)))

    def vec_mismatch(self, curve, a, b, n, result, a_stride=1, b_stride=1, first=0):
        """cg_vec_mismatch_dev: the positions first <= i < n with a[i * a_stride] != b[i * b_stride] (b None: != 0); result = 16-byte device buffer
        (count, first differing position)"""
        _chk(load().cg_vec_mismatch_dev(self.h, curve, _dp(a), C.c_size_t(a_stride), _dp(b), C.c_size_t(b_stride), C.c_size_t(first), C.c_size_t(n), _dp(result)))

    def spmv_csr(self, curve, row_ptr, col, coeff, n_rows, pub, n_inputs, party, wit_a, wit_b, out_a, out_b):
        _chk(load().cg_spmv_csr_dev(self.h, curve, _dp(row_ptr), _dp(col), _dp(coeff), C.c_size_t(n_rows), _dp(pub), C.c_uint32(n_inputs), int(party),
                                    _dp(wit_a), _dp(wit_b), _dp(out_a), _dp(out_b)))

    # ---- host-buffer forms
    def vec_mul_host(self, curve, a, b):
        a = np.ascontiguousarray(a, dtype=np.uint64); b = np.ascontiguousarray(b, dtype=np.uint64)
        out = np.empty_like(a)
        _chk(load().cg_vec_mul(self.h, curve, _hp(out), _hp(a), _hp(b), C.c_size_t(a.size // 4)))
        return out

    def vec_rep3_mul_local_host(self, curve, aa, ab, ba, bb, mask=None):
        arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (aa, ab, ba, bb)]
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint64)
        out = np.empty_like(arrs[0])
        _chk(load().cg_vec_rep3_mul_local(self.h, curve, _hp(out), *[_hp(x) for x in arrs], _hp(m), C.c_size_t(arrs[0].size // 4)))
        return out

    # ---- stats
    def stats_enable(self, on=True): _chk(load().cg_stats_enable(self.h, int(on)))

    def stats(self, reset=False):
        class ST(C.Structure):
            _fields_ = [("msm_ms", C.c_double), ("ntt_ms", C.c_double), ("vec_ms", C.c_double), ("spmv_ms", C.c_double),
                        ("msm_calls", C.c_uint64), ("ntt_calls", C.c_uint64), ("vec_calls", C.c_uint64), ("spmv_calls", C.c_uint64),
                        ("msm_sort_ms", C.c_double), ("msm_acc_g1_ms", C.c_double), ("msm_acc_g2_ms", C.c_double), ("msm_reduce_ms", C.c_double),
                        ("msm_sort_calls", C.c_uint64), ("msm_acc_g1_calls", C.c_uint64), ("msm_acc_g2_calls", C.c_uint64), ("msm_reduce_calls", C.c_uint64)]
        st = ST()
        _chk(load().cg_stats(self.h, C.byref(st), int(reset)))
        return {f: getattr(st, f) for f, _ in ST._fields_}


# ---- O(1) host helpers (no device needed) --------------------------------------------------------------
def dev_cache_trim(device=0):
    """give the device blocks parked by cg_dev_free back to the runtime (call when the device is idle); returns the bytes released"""
    n = C.c_size_t(0)
    _chk(load().cg_dev_cache_trim(int(device), C.byref(n)))
    return int(n.value)


def device_count():
    """HIP devices visible to the library (0 without a GPU)"""
    return int(load().cg_device_count())


def session_devices(world):
    """device list of a `world`-device session on THIS box: distinct GPUs as far as they exist, then repeats (a one-GPU box runs every
    context on GPU 0; on a node the hops between devices are real peer copies over xGMI)"""
    n = max(1, device_count())
    return [i % n for i in range(world)]


def set_option(option, value):
    """process-wide option of the hip library (cg_set_option)"""
    _chk(load().cg_set_option(int(option), C.c_int64(int(value))))


def get_option(option):
    v = C.c_int64(0)
    _chk(load().cg_get_option(int(option), C.byref(v)))
    return v.value


PREFLIGHT_ALLOW_SHARED, PREFLIGHT_ALLOW_STAGED = 1, 2


def device_preflight(devices, allow_shared=False, allow_staged=False):
    """cg_device_preflight: raises BackendError unless `devices` are distinct GPUs with peer access whose pairwise 1 MiB copies arrive intact;
    returns the report (bus ids, per-pair peer access and copy rate) as a dict"""
    import json
    devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
    buf = C.create_string_buffer(1 << 16)
    _chk(load().cg_device_preflight(devs, len(devices), C.c_uint32((1 if allow_shared else 0) | (2 if allow_staged else 0)), buf, C.c_size_t(len(buf))))
    return json.loads(buf.value.decode())


def point_add(curve, group, a, b):
    out = np.zeros(point_words(curve, group, 3), dtype=np.uint64)
    _chk(load().cg_point_add(curve, group, _hp(np.ascontiguousarray(a)), _hp(np.ascontiguousarray(b)), _hp(out)))
    return out


def point_neg(curve, group, a):
    out = np.zeros(point_words(curve, group, 3), dtype=np.uint64)
    _chk(load().cg_point_neg(curve, group, _hp(np.ascontiguousarray(a)), _hp(out)))
    return out


def point_scalar_mul(curve, group, a, k):
    out = np.zeros(point_words(curve, group, 3), dtype=np.uint64)
    _chk(load().cg_point_scalar_mul(curve, group, _hp(np.ascontiguousarray(a)), _hp(np.ascontiguousarray(k)), _hp(out)))
    return out


class FixedBase:
    """8-bit window table of one base point (cg_fixed_base_*): host arithmetic, no device"""

    def __init__(self, curve, group, point_jacobian):
        self.curve, self.group, self.h = curve, group, C.c_void_p()
        p = np.ascontiguousarray(point_jacobian, dtype=np.uint64)
        _chk(load().cg_fixed_base_create(curve, group, _hp(p), C.byref(self.h)))

    def mul(self, k):
        out = np.zeros(point_words(self.curve, self.group, 3), dtype=np.uint64)
        _chk(load().cg_fixed_base_mul(self.h, _hp(np.ascontiguousarray(k, dtype=np.uint64)), _hp(out)))
        return out

    def close(self):
        if self.h: load().cg_fixed_base_destroy(self.h); self.h = None

    def __del__(self):
        try: self.close()
        except Exception: pass


def point_generator(curve, group):
    out = np.zeros(point_words(curve, group, 3), dtype=np.uint64)
    _chk(load().cg_point_generator(curve, group, _hp(out)))
    return out


def point_validate(curve, group, affine):
    """the reference's checks on a deserialised point (coordinates below the modulus, on the curve, in the subgroup); host arithmetic"""
    ok = C.c_int32(0)
    _chk(load().cg_point_validate(curve, group, _hp(np.ascontiguousarray(affine, dtype=np.uint64)), C.byref(ok)))
    return bool(ok.value)


def fr_is_canonical(curve, elements):
    e = np.ascontiguousarray(elements, dtype=np.uint64).reshape(-1, 4)
    ok = C.c_int32(0)
    _chk(load().cg_fr_is_canonical(curve, _hp(e), C.c_size_t(e.shape[0]), C.byref(ok)))
    return bool(ok.value)


def point_to_affine(curve, group, a):
    out = np.zeros(point_words(curve, group, 2), dtype=np.uint64)
    _chk(load().cg_point_to_affine(curve, group, _hp(np.ascontiguousarray(a)), _hp(out)))
    return out


def point_from_affine(curve, group, a):
    out = np.zeros(point_words(curve, group, 3), dtype=np.uint64)
    _chk(load().cg_point_from_affine(curve, group, _hp(np.ascontiguousarray(a)), _hp(out)))
    return out


def fr_op(curve, op, a, b=None):
    out = np.zeros(4, dtype=np.uint64)
    _chk(load().cg_fr_op(curve, {"add": 0, "sub": 1, "mul": 2, "inv": 3}[op], _hp(np.ascontiguousarray(a)), _hp(None if b is None else np.ascontiguousarray(b)), _hp(out)))
    return out


# ---- pairing on the host (cg_pairing ...): target-field elements are (2, 3, 2, limbs) u64, Montgomery, the layout of vk_alphabeta_12
def _pairs(curve, g1, g2):
    nq = fq_limbs(curve)
    g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(-1, 2 * nq); g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(-1, 4 * nq)
    assert g1.shape[0] == g2.shape[0], "as many G1 as G2 points"
    return g1, g2


def pairing(curve, g1_affine, g2_affine):
    """e(P, Q) with arkworks' / snarkjs' value convention; host arithmetic, no device"""
    g1, g2 = _pairs(curve, g1_affine, g2_affine)
    out = np.zeros((2, 3, 2, fq_limbs(curve)), dtype=np.uint64)
    _chk(load().cg_pairing(curve, _hp(g1), _hp(g2), _hp(out)))
    return out


def final_exp(curve, value):
    out = np.zeros((2, 3, 2, fq_limbs(curve)), dtype=np.uint64)
    _chk(load().cg_final_exp(curve, _hp(np.ascontiguousarray(value, dtype=np.uint64)), _hp(out)))
    return out


def fp12_mul(curve, a, b):
    out = np.zeros((2, 3, 2, fq_limbs(curve)), dtype=np.uint64)
    _chk(load().cg_fp12_mul(curve, _hp(np.ascontiguousarray(a, dtype=np.uint64)), _hp(np.ascontiguousarray(b, dtype=np.uint64)), _hp(out)))
    return out


def fp12_pow(curve, a, exponent):
    """a^exponent for a non-negative Python integer"""
    nl = max(1, (int(exponent).bit_length() + 63) // 64)
    e = np.array([(int(exponent) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(nl)], dtype=np.uint64)
    out = np.zeros((2, 3, 2, fq_limbs(curve)), dtype=np.uint64)
    _chk(load().cg_fp12_pow(curve, _hp(np.ascontiguousarray(a, dtype=np.uint64)), _hp(e), nl, _hp(out)))
    return out


def fp12_one(curve):
    """the target field's one: the Miller value of no pairs"""
    return miller_loop(curve, np.zeros((0, 2 * fq_limbs(curve)), dtype=np.uint64), np.zeros((0, 4 * fq_limbs(curve)), dtype=np.uint64))


def miller_loop(curve, g1, g2):
    """product of the Miller values of the pairs, no final exponentiation; host arithmetic"""
    g1, g2 = _pairs(curve, g1, g2)
    out = np.zeros((2, 3, 2, fq_limbs(curve)), dtype=np.uint64)
    _chk(load().cg_miller_loop(curve, _hp(g1), _hp(g2), C.c_size_t(g1.shape[0]), _hp(out)))
    return out


def pairing_check(curve, g1, g2):
    """prod e(g1[i], g2[i]) == 1 with one final exponentiation; host arithmetic"""
    g1, g2 = _pairs(curve, g1, g2)
    ok = C.c_int32(0)
    _chk(load().cg_pairing_check(curve, _hp(g1), _hp(g2), C.c_size_t(g1.shape[0]), C.byref(ok)))
    return bool(ok.value)


# ---- Plonk verification, the per-proof layer (cg_plonk_verify_scalars{,_host}; csrc/plonk_verify.hpp) -----------------------------------
def _plonk_verify_scalars(ctx_handle, curve, key, commits, evals, pubs, coeff128):
    nq = fq_limbs(curve)
    commits = np.ascontiguousarray(commits, dtype=np.uint64).reshape(-1, 9, 2 * nq)
    n = commits.shape[0]
    evals = np.ascontiguousarray(evals, dtype=np.uint64).reshape(n, 6, 4)
    pubs = np.ascontiguousarray(pubs, dtype=np.uint64).reshape(n, -1, 4) if np.size(pubs) else np.zeros((n, 0, 4), dtype=np.uint64)
    n_pub = pubs.shape[1]
    if coeff128 is not None:
        coeff128 = np.ascontiguousarray(coeff128, dtype=np.uint64).reshape(n, 2)
    pts = np.ascontiguousarray(key["points"], dtype=np.uint64).reshape(8, 2 * nq)
    ch = np.zeros((n, 6, 4), dtype=np.uint64); sp = np.zeros((n, 11, 4), dtype=np.uint64); sk = np.zeros((n, 9, 4), dtype=np.uint64)
    valid = np.zeros(max(n, 1), dtype=np.int32); sums = np.zeros((9, 4), dtype=np.uint64)
    args = (curve, _hp(pts), _hp(_fa(key["k1"])), _hp(_fa(key["k2"])), _hp(_fa(key["omega"])), int(key["power"]), _hp(commits), _hp(evals), _hp(pubs),
            C.c_size_t(n_pub), C.c_size_t(n), _hp(coeff128), _hp(ch), _hp(sp), _hp(sk), _hp(valid), _hp(sums))
    if ctx_handle is None:
        _chk(load().cg_plonk_verify_scalars_host(*args))
    else:
        _chk(load().cg_plonk_verify_scalars(ctx_handle, *args))
    return dict(challenges=ch, proof_scalars=sp, key_scalars=sk, valid=valid[:n].copy(), key_sums=sums)


def plonk_verify_scalars_host(curve, key, commits, evals, pubs, coeff128=None):
    """The Fiat-Shamir challenges and the scalars of n Plonk proofs under one key, on the host (the function the GPU lanes run).
    key: dict(points=(8, point words) Qm..S3, k1, k2, omega, power); commits (n, 9, point words); evals (n, 6, 4); pubs (n, n_pub, 4);
    coeff128 (optional): (n, 2) u64, canonical 128-bit integers multiplied into every scalar of their proof.
    Returns dict(challenges (n, 6, 4): beta, gamma, alpha, xi, v, u; proof_scalars (n, 11, 4); key_scalars (n, 9, 4); valid (n); key_sums (9, 4))."""
    return _plonk_verify_scalars(None, curve, key, commits, evals, pubs, coeff128)


# ---- host-side mirror of the reference prover interface (libcogroth16_host.so, C++ over the C ABI) -----------------------
_host = None


def load_host():
    global _host
    if _host is None:
        load()
        if not os.path.exists(HOST_LIB_PATH):
            raise BackendError(f"{HOST_LIB_PATH} is missing: build it with `make -C collaborative-circom_amd/host`")
        _host = C.CDLL(HOST_LIB_PATH)
        _host.cgh_last_error.restype = C.c_char_p
    return _host


def _hchk(rc):
    if rc != 0:
        raise BackendError("cogroth16_host: " + load_host().cgh_last_error().decode())


def host_zkey_info(curve, path):
    info = (C.c_size_t * 7)()
    _hchk(load_host().cgh_zkey_info(curve, path.encode(), info))
    keys = ("n_vars", "n_public", "domain_size", "pow", "num_constraints", "nnz_a", "nnz_b")
    return dict(zip(keys, [int(x) for x in info]))


def host_zkey_validate(curve, path, device=0):
    """zkey -> device with the parser's per-point validation on the GPU; raises BackendError naming the first bad point.
    Returns (host seconds for read + decode, device seconds for upload + validation)."""
    secs = (C.c_double * 2)()
    _hchk(load_host().cgh_zkey_validate(int(device), curve, path.encode(), secs))
    return float(secs[0]), float(secs[1])


def host_proof_to_json(curve, proof):
    """Groth16Proof JSON text (proof.rs:8-29) of a packed proof A || B || C"""
    buf = C.create_string_buffer(4096)
    _hchk(load_host().cgh_proof_to_json(curve, _hp(np.ascontiguousarray(proof, dtype=np.uint64)), buf, C.c_size_t(4096)))
    return buf.value.decode()


def host_proof_from_json(curve, text):
    nq = 6 if curve == BLS12_381 else 4
    out = np.zeros(8 * nq, dtype=np.uint64)
    _hchk(load_host().cgh_proof_from_json(curve, text.encode(), _hp(out)))
    return out


def host_public_to_json(curve, pub):
    """public.json text (co-circom.rs:620-628) of n public signals in Montgomery form (without the leading constant 1)"""
    pub = np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 4)
    buf = C.create_string_buffer(96 * max(1, pub.shape[0]) + 16)
    _hchk(load_host().cgh_public_to_json(curve, _hp(pub), C.c_size_t(pub.shape[0]), buf, C.c_size_t(len(buf))))
    return buf.value.decode()


def prove_shamir(curve, zkey_path, n, t, pub, wits, streams, device=0, want_h=False, preprocess=0):
    """n Shamir parties (threads) with threshold t on one GPU; returns (n proofs[, party 0's h shares]).  preprocess = number of
    secrets every party double-shares up front on the GPU (ShamirProtocol::preprocess); 0 = the reference's lazy batches of 1024."""
    info = host_zkey_info(curve, zkey_path)
    nq = 6 if curve == BLS12_381 else 4
    out = np.zeros((n, 8 * nq), dtype=np.uint64)
    h = np.zeros((info["domain_size"], 4), dtype=np.uint64) if want_h else None
    keep = [[np.ascontiguousarray(x, dtype=np.uint64) for x in lst] for lst in (wits, streams)]
    arr = lambda lst: (C.c_void_p * n)(*[x.ctypes.data for x in lst])
    _hchk(load_host().cgh_prove_shamir(int(device), curve, zkey_path.encode(), int(n), int(t), _hp(np.ascontiguousarray(pub, dtype=np.uint64)),
                                       arr(keep[0]), arr(keep[1]), C.c_size_t(keep[1][0].shape[0]), C.c_size_t(int(preprocess)), _hp(out), _hp(h) if want_h else None))
    return (out, h) if want_h else out


def host_synth_circuit(curve, log_m, seed, zkey_path, wtns_path, device=0):
    """synthetic satisfiable circuit of 2^log_m - 2 constraints with a valid Groth16 CRS (toxic waste from `seed`, point tables by
    fixed-base batch multiplication on the GPU), written as snarkjs-format .zkey + .wtns files (bench / test tooling)"""
    _hchk(load_host().cgh_synth_circuit(int(device), curve, int(log_m), C.c_uint64(seed), zkey_path.encode(), wtns_path.encode()))


def host_synth_plonk_circuit(curve, log_n, seed, zkey_path, wtns_path, n_public=1, n_additions=0, device=0):
    """synthetic satisfiable Plonk circuit of domain 2^log_n (toxic waste from `seed`, p_tau by fixed-base batch multiplication and the
    polynomials' evaluations by the library's NTT on the GPU), written as a snarkjs-format Plonk .zkey + .wtns (bench / test tooling)"""
    _hchk(load_host().cgh_synth_plonk_circuit(int(device), curve, int(log_n), C.c_uint64(seed), C.c_uint32(n_public), C.c_uint32(n_additions),
                                              zkey_path.encode(), wtns_path.encode()))


NO_ROW = (1 << 64) - 1


class R1cs:
    """an iden3 .r1cs file (cgh_r1cs_*): the three constraint matrices, the zkey coefficient section they determine, the witness check on the GPU"""

    def __init__(self, curve, path):
        h = C.c_void_p()
        _hchk(load_host().cgh_r1cs_open(curve, path.encode(), C.byref(h)))
        self.curve, self.h = curve, h
        info = (C.c_size_t * 7)()
        _hchk(load_host().cgh_r1cs_info(self.h, info))
        self.info = dict(zip(("n_wires", "n_public", "n_constraints", "domain_size", "nnz_a", "nnz_b", "nnz_c"), [int(x) for x in info]))

    def close(self):
        if self.h: load_host().cgh_r1cs_close(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def coeff_section(self):
        """section 4 of the Groth16 zkey of this circuit, as bytes (host only)"""
        n = C.c_size_t(0)
        _hchk(load_host().cgh_r1cs_coeff_section(self.h, None, C.c_size_t(0), C.byref(n)))
        buf = (C.c_uint8 * n.value)()
        _hchk(load_host().cgh_r1cs_coeff_section(self.h, buf, C.c_size_t(n.value), C.byref(n)))
        return bytes(buf)

    def check_witness(self, witness, device=0, form=0):
        """(n_bad, first_bad) of the plain full witness (n_wires Montgomery elements): the number of constraints it violates and the smallest
        such row, NO_ROW when it satisfies the circuit.  form: 0 = kernel form chosen by size, 1 = a lane per row, 2 = a wave per row."""
        w = np.ascontiguousarray(witness, dtype=np.uint64).reshape(-1, 4)
        if w.shape[0] != self.info["n_wires"]:
            raise BackendError(f"cogroth16_host: a witness of {w.shape[0]} values for a circuit of {self.info['n_wires']} wires")
        n_bad, first = C.c_uint64(0), C.c_uint64(0)
        _hchk(load_host().cgh_r1cs_check_witness_form(int(device), self.h, int(form), _hp(w), C.byref(n_bad), C.byref(first)))
        return int(n_bad.value), int(first.value)

    def plonk_info(self, device=0):
        """sizes of the Plonk key of this circuit (cgh_r1cs_plonk_info, the count pass of the gate compiler on the GPU): dict of n_additions,
        n_constraints, n_vars, domain_size"""
        out = (C.c_size_t * 4)()
        _hchk(load_host().cgh_r1cs_plonk_info(int(device), self.h, out))
        return dict(zip(("n_additions", "n_constraints", "n_vars", "domain_size"), [int(x) for x in out]))


    def plonk_gate_origin(self, row, device=0):
        """where gate row `row` of this circuit's Plonk key comes from (cgh_r1cs_plonk_gate_origin): (kind, R1CS row, index of the addition
        within that row), kind one of PLONK_GATE_PUBLIC / _ADDITION / _CONSTRAINT / _PADDING, None where a field does not apply"""
        out = (C.c_uint64 * 3)()
        _hchk(load_host().cgh_r1cs_plonk_gate_origin(int(device), self.h, C.c_uint64(row), out))
        return int(out[0]), (None if out[1] == NO_ROW else int(out[1])), (None if out[2] == NO_ROW else int(out[2]))


PLONK_GATE_PUBLIC, PLONK_GATE_ADDITION, PLONK_GATE_CONSTRAINT, PLONK_GATE_PADDING = 0, 1, 2, 3
# the checks of PlonkSession.audit (CGH_PLONK_AUDIT_*), one bit each, in the order of the detail pairs
PLONK_AUDIT_HEADER, PLONK_AUDIT_BLOCKS, PLONK_AUDIT_ROWS, PLONK_AUDIT_SIGMA, PLONK_AUDIT_COMMITMENTS, PLONK_AUDIT_SRS, PLONK_AUDIT_CIRCUIT = 1, 2, 4, 8, 16, 32, 64
PLONK_AUDIT_NAMES = ("HEADER", "BLOCKS", "ROWS", "SIGMA", "COMMITMENTS", "SRS", "CIRCUIT")
PLONK_AUDIT_STAGES = ("header", "transforms", "comparisons", "msm_commitments", "msm_srs", "pairing", "circuit")


def setup_groth16(r1cs, seed, zkey_path, device=0):
    """a snarkjs-format Groth16 .zkey for the circuit from seeded toxic waste (cgh_setup_groth16_dev), computed on the GPU.
    DEVELOPMENT ONLY: whoever holds the seed can forge proofs for this key."""
    _hchk(load_host().cgh_setup_groth16_dev(int(device), r1cs.h, C.c_uint64(seed), zkey_path.encode()))


PLONK_SETUP_STAGES = ("count", "emit", "sigma", "transforms", "points", "lagrange", "write")


def setup_plonk(r1cs, seed, zkey_path, device=0, timing=False):
    """a snarkjs-format Plonk .zkey for the circuit (cgh_setup_plonk_dev): gates, permutation and polynomials as snarkjs' `plonk setup` makes
    them, computed on the GPU; the points from tau = setup_toxic(curve, seed)[0].  timing=True returns the seconds per stage
    (PLONK_SETUP_STAGES, through cgh_setup_plonk_tau_dev).
    DEVELOPMENT ONLY: the seed is the toxic waste, whoever holds it can forge proofs for this key."""
    if timing:
        return setup_plonk_tau(r1cs, setup_toxic(r1cs.curve, seed)[0], zkey_path, device=device, timing=True)
    _hchk(load_host().cgh_setup_plonk_dev(int(device), r1cs.h, C.c_uint64(seed), None if zkey_path is None else zkey_path.encode()))


def setup_plonk_tau(r1cs, tau, zkey_path, device=0, timing=False):
    """setup_plonk with tau given (4 Montgomery limbs) instead of drawn from a seed (cgh_setup_plonk_tau_dev).  DEVELOPMENT ONLY."""
    secs = (C.c_double * len(PLONK_SETUP_STAGES))() if timing else None
    _hchk(load_host().cgh_setup_plonk_tau_dev(int(device), r1cs.h, _hp(np.ascontiguousarray(tau, dtype=np.uint64).reshape(4)), zkey_path.encode(), secs))
    return dict(zip(PLONK_SETUP_STAGES, secs)) if timing else None


def setup_toxic(curve, seed):
    """tau, alpha, beta, gamma, delta of setup_groth16 for a seed, Montgomery (5, 4)"""
    out = np.zeros((5, 4), dtype=np.uint64)
    _hchk(load_host().cgh_setup_toxic(curve, C.c_uint64(seed), _hp(out)))
    return out


def host_set_zkey_validation(on):
    """the prove entry points and session_open validate every zkey point on the GPU by default (the reference's parser does);
    callers that validated the file before can switch it off"""
    _hchk(load_host().cgh_set_zkey_validation(int(bool(on))))


# process-wide options of the host library (include/cogroth16_host.h: cgh_set_option)
HOST_OPT_XCHG_ASYNC_MIN, HOST_OPT_DEVICE_MASKS_MIN, HOST_OPT_XCHG_COPY_STREAM_MIN, HOST_OPT_SECOND_CONTEXT_MIN_LOG, HOST_OPT_DISTRIBUTED_MAP, HOST_OPT_ONE_CONTEXT, HOST_OPT_SPLIT_FIRST_MSM_MIN, HOST_OPT_CTX_WIDE_LOG, HOST_OPT_CTX_OFF_MAIN_LOG, HOST_OPT_CTX_SOLO_LOG = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10


def host_set_option(option, value):
    _hchk(load_host().cgh_set_option(int(option), C.c_int64(int(value))))


def host_get_option(option):
    v = C.c_int64(0)
    _hchk(load_host().cgh_get_option(int(option), C.byref(v)))
    return v.value


class host_options:
    """with cg.host_options({cg.HOST_OPT_XCHG_ASYNC_MIN: 4096}): ... — set for the block, restored afterwards (tests)"""

    def __init__(self, values):
        self.values, self.saved = dict(values), {}

    def __enter__(self):
        for k, v in self.values.items():
            self.saved[k] = host_get_option(k); host_set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            host_set_option(k, v)
        return False


class ProvingSession:
    """zkey read, uploaded and (optionally) given per-window precomputed tables once; proofs then cost what co-circom.rs:503-506 times"""

    def __init__(self, curve, zkey_path, precompute=True, device=0, validate=True, devices=None, additive_h=False, shared_devices=False):
        """devices: several GPUs of one node for this party (cgh_session_open_multi): devices[0] runs the witness map and slice 0 of
        every MSM, devices[i] slice i.  additive_h: REP3 proofs run the additive-quotient variant (CGH_SESSION_ADDITIVE_H, opt-in: not the
        reference's message sequence, same proof).  shared_devices: the list may name one GPU several times (CGH_SESSION_SHARED_DEVICES:
        one-GPU tests and planning runs) — without it a multi-device session opens only on DISTINCT GPUs that pass cg_device_preflight"""
        self.curve, self.info = curve, host_zkey_info(curve, zkey_path)
        h = C.c_void_p()
        devs = [int(device)] if devices is None else [int(d) for d in devices]
        arr = (C.c_int32 * len(devs))(*devs)
        _hchk(load_host().cgh_session_open_multi(arr, len(devs), curve, zkey_path.encode(), -1 if precompute is True else int(precompute), C.c_uint32((0 if validate else 1) | (2 if additive_h else 0) | (4 if shared_devices else 0)), C.byref(h)))
        self.h = h

    def close(self):
        if self.h: load_host().cgh_session_close(self.h); self.h = None

    def prove_plain(self, witness, r, s):
        """returns (proof, seconds)"""
        nq = 6 if self.curve == BLS12_381 else 4
        out = np.zeros(8 * nq, dtype=np.uint64); sec = (C.c_double * 1)()
        _hchk(load_host().cgh_session_prove_plain(self.h, _hp(np.ascontiguousarray(witness, dtype=np.uint64)), _hp(np.ascontiguousarray(r, dtype=np.uint64)),
                                                  _hp(np.ascontiguousarray(s, dtype=np.uint64)), _hp(out), sec))
        return out, sec[0]

    def verify(self, proof, pub):
        """Groth16::verify of a proof against the session's own key (cgh_session_verify); pub = the n_public public inputs, Montgomery"""
        ok = C.c_int32(0)
        pub = np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 4)
        if pub.shape[0] != self.info["n_public"]:
            raise BackendError(f"cogroth16_host: {pub.shape[0]} public inputs for a key with {self.info['n_public']}")
        _hchk(load_host().cgh_session_verify(self.h, _hp(np.ascontiguousarray(proof, dtype=np.uint64)), _hp(pub), C.byref(ok)))
        return bool(ok.value)

    def prove_rep3(self, pub, wit_a, wit_b, streams, solo=True):
        """three co-located parties; returns (3 proofs, seconds of the three together, seconds of party 0 replayed alone on the GPU)"""
        nq = 6 if self.curve == BLS12_381 else 4
        out = np.zeros((3, 8 * nq), dtype=np.uint64); sec = (C.c_double * 2)()
        keep = [[np.ascontiguousarray(x, dtype=np.uint64) for x in lst] for lst in (wit_a, wit_b, streams)]
        arr = lambda lst: (C.c_void_p * 3)(*[x.ctypes.data for x in lst])
        _hchk(load_host().cgh_session_prove_rep3(self.h, _hp(np.ascontiguousarray(pub, dtype=np.uint64)), arr(keep[0]), arr(keep[1]), arr(keep[2]),
                                                 C.c_size_t(keep[2][0].shape[0]), _hp(out), sec if solo else None))
        return out, sec[0], sec[1]


class VerifyingKey:
    """Groth16 verifying key (cgh_vk_*): points validated, e(alpha, beta), -gamma and -delta prepared when the handle is opened"""

    def __init__(self, curve, handle):
        self.curve, self.h = curve, handle
        info = (C.c_size_t * 2)()
        _hchk(load_host().cgh_vk_info(self.h, info))
        self.n_public = int(info[1])

    @classmethod
    def from_json(cls, curve, path):
        h = C.c_void_p()
        _hchk(load_host().cgh_vk_from_json(curve, path.encode(), C.byref(h)))
        return cls(curve, h)

    @classmethod
    def from_zkey(cls, curve, path):
        h = C.c_void_p()
        _hchk(load_host().cgh_vk_from_zkey(curve, path.encode(), C.byref(h)))
        return cls(curve, h)

    def close(self):
        if self.h: load_host().cgh_vk_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alphabeta(self):
        """the prepared e(alpha_1, beta_2) as (2, 3, 2, limbs): the layout of vk_alphabeta_12"""
        out = np.zeros((2, 3, 2, fq_limbs(self.curve)), dtype=np.uint64)
        _hchk(load_host().cgh_vk_alphabeta(self.h, _hp(out)))
        return out

    def verify(self, proof, pub):
        """one proof on the host (cgh_groth16_verify); a wrong number of public inputs or a non-canonical one raises BackendError"""
        pub = np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 4)
        ok = C.c_int32(0)
        _hchk(load_host().cgh_groth16_verify(self.h, _hp(np.ascontiguousarray(proof, dtype=np.uint64)), _hp(pub), C.c_size_t(pub.shape[0]), C.byref(ok)))
        return bool(ok.value)

    def verify_batch(self, proofs, pubs, seed=None, per_proof=False, device=0, timing=False):
        """n proofs on the GPU with random 128-bit coefficients (cgh_groth16_verify_batch).  proofs: (n, proof words); pubs: (n, n_public, 4).
        Returns the verdict; with per_proof=True (verdict, flags); with timing=True the five stage times in seconds are appended."""
        nq = fq_limbs(self.curve)
        proofs = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8 * nq)
        n = proofs.shape[0]
        pubs = np.ascontiguousarray(pubs, dtype=np.uint64).reshape(n, self.n_public, 4) if n else np.zeros((0, self.n_public, 4), dtype=np.uint64)
        ok = C.c_int32(0)
        flags = np.zeros(max(n, 1), dtype=np.uint8) if per_proof else None
        secs = (C.c_double * 5)()
        _hchk(load_host().cgh_groth16_verify_batch_timed(int(device), self.h, _hp(proofs), _hp(pubs), C.c_size_t(pubs.shape[1]), C.c_size_t(n),
                                                         None if seed is None else bytes(seed), C.byref(ok), _hp(flags), secs))
        out = (bool(ok.value),) + ((flags[:n].astype(bool),) if per_proof else ()) + ((list(secs),) if timing else ())
        return out[0] if len(out) == 1 else out


# ---- one REP3 party with the caller's network and randomness (cgh_session_prove_rep3_party) ------------------------------------
_SEND = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t)
_RECV = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t)
_RECV_PINNED = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


class Rep3NetTable(C.Structure):
    """cgh_rep3_net (include/cogroth16_host.h): the party's channels to its two peers"""
    _fields_ = [("user", C.c_void_p), ("party_id", C.c_int32), ("send_next", _SEND), ("recv_prev", _RECV), ("send_prev", _SEND), ("recv_next", _RECV),
                ("recv_prev_pinned", _RECV_PINNED)]


_MASKS = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p))
_FES = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_EC = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_void_p)


class Rep3RandTable(C.Structure):
    """cgh_rep3_rand: the party's correlated randomness (Rep3Rand, rep3/rngs.rs:25-62)"""
    _fields_ = [("user", C.c_void_p), ("masking_field_elements", _MASKS), ("random_fes", _FES), ("masking_ec_element", _EC)]


class LoopbackHub:
    """three parties of one process joined by in-memory queues (cgh_loopback_*); net(i) is party i's callback table"""

    def __init__(self):
        self.h = C.c_void_p(); _hchk(load_host().cgh_loopback_create(C.byref(self.h)))

    def net(self, party, record=False):
        t = Rep3NetTable(); _hchk(load_host().cgh_loopback_net(self.h, int(party), int(bool(record)), C.byref(t))); return t

    def replay_net(self, party):
        t = Rep3NetTable(); _hchk(load_host().cgh_loopback_replay_net(self.h, int(party), C.byref(t))); return t

    def abort(self): load_host().cgh_loopback_abort(self.h)

    def close(self):
        if self.h: load_host().cgh_loopback_destroy(self.h); self.h = None


class StreamRand:
    """Rep3Rand over two pre-generated streams of field elements (cgh_stream_rand_create); .table is the callback table"""

    def __init__(self, curve, rng1, rng2):
        self.keep = (np.ascontiguousarray(rng1, dtype=np.uint64), np.ascontiguousarray(rng2, dtype=np.uint64))
        self.h = C.c_void_p(); self.table = Rep3RandTable()
        _hchk(load_host().cgh_stream_rand_create(curve, _hp(self.keep[0]), _hp(self.keep[1]), C.c_size_t(self.keep[0].shape[0]), C.byref(self.h), C.byref(self.table)))

    def close(self):
        if self.h: load_host().cgh_stream_rand_destroy(self.h); self.h = None


_CH_STATE = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64))
_CH_SETPOS = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_uint64, C.c_uint64)


class Rep3ChaChaTable(C.Structure):
    """cgh_rep3_chacha: seeds and word positions of Rep3Rand's two ChaCha12 generators, so that the masking vectors are drawn on the GPU"""
    _fields_ = [("user", C.c_void_p), ("get_state", _CH_STATE), ("set_word_pos", _CH_SETPOS)]


class ChaChaRand:
    """Rep3Rand over two ChaCha12 generators (cgh_chacha_rand_create): .table = the O(1) / host callbacks, .streams = the generator description"""

    def __init__(self, curve, seed1, seed2):
        self.h = C.c_void_p(); self.table = Rep3RandTable(); self.streams = Rep3ChaChaTable()
        _hchk(load_host().cgh_chacha_rand_create(curve, bytes(seed1), bytes(seed2), C.byref(self.h), C.byref(self.table), C.byref(self.streams)))

    def positions(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        _hchk(load_host().cgh_chacha_rand_positions(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.h: load_host().cgh_chacha_rand_destroy(self.h); self.h = None


def chacha12_fr_rand_host(curve, seed, word_pos, n):
    """n x F::rand over ChaCha12Rng::from_seed(seed) at word_pos, on the host (one thread): (n x 4 limbs, word position afterwards)"""
    out = np.zeros((n, 4), dtype=np.uint64); after = C.c_uint64(0)
    _hchk(load_host().cgh_chacha12_fr_rand_host(curve, bytes(seed), C.c_uint64(word_pos), C.c_size_t(n), _hp(out), C.byref(after)))
    return out, after.value


_SH_SEND = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t)
_SH_RECV = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t)
_SH_RAND = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p)


class ShamirNetTable(C.Structure):
    """cgh_shamir_net: any-to-any channels of one of n parties (shamir/network.rs:17-59)"""
    _fields_ = [("user", C.c_void_p), ("party_id", C.c_int32), ("num_parties", C.c_int32), ("send", _SH_SEND), ("recv", _SH_RECV)]


class ShamirRandTable(C.Structure):
    """cgh_shamir_rand: the party's private RNG (F::rand draws in the reference's order)"""
    _fields_ = [("user", C.c_void_p), ("random_field_elements", _SH_RAND)]


class ShamirLoopbackHub:
    """n Shamir parties of one process joined by in-memory queues (cgh_shamir_loopback_*); net(i) is party i's callback table"""

    def __init__(self, n):
        self.h = C.c_void_p(); _hchk(load_host().cgh_shamir_loopback_create(int(n), C.byref(self.h)))

    def net(self, party, record=False):
        t = ShamirNetTable(); _hchk(load_host().cgh_shamir_loopback_net(self.h, int(party), int(bool(record)), C.byref(t))); return t

    def replay_net(self, party):
        t = ShamirNetTable(); _hchk(load_host().cgh_shamir_loopback_replay_net(self.h, int(party), C.byref(t))); return t

    def abort(self): load_host().cgh_shamir_loopback_abort(self.h)

    def close(self):
        if self.h: load_host().cgh_shamir_loopback_destroy(self.h); self.h = None


def host_prove_shamir_party(session, threshold, pub, wit, net_table, rand_table, preprocess=0):
    """ONE Shamir party on an open ProvingSession through the callback ABI; returns (proof, seconds).  Call it from one thread per party."""
    nq = 6 if session.curve == BLS12_381 else 4
    out = np.zeros(8 * nq, dtype=np.uint64); sec = (C.c_double * 1)()
    keep = [np.ascontiguousarray(x, dtype=np.uint64) for x in (pub, wit)]
    _hchk(load_host().cgh_session_prove_shamir_party(session.h, int(threshold), _hp(keep[0]), _hp(keep[1]), C.byref(net_table), C.byref(rand_table),
                                                     C.c_size_t(int(preprocess)), _hp(out), sec))
    return out, sec[0]


def host_prove_shamir_party_seeded(session, threshold, pub, wit, net_table, seed, preprocess=0):
    """ONE Shamir party whose private randomness is a ChaCha12 generator run by the library from `seed` (32 bytes); returns (proof, seconds)"""
    nq = 6 if session.curve == BLS12_381 else 4
    out = np.zeros(8 * nq, dtype=np.uint64); sec = (C.c_double * 1)()
    keep = [np.ascontiguousarray(x, dtype=np.uint64) for x in (pub, wit)]
    _hchk(load_host().cgh_session_prove_shamir_party_seeded(session.h, int(threshold), _hp(keep[0]), _hp(keep[1]), C.byref(net_table), bytes(seed),
                                                            C.c_size_t(int(preprocess)), _hp(out), sec))
    return out, sec[0]


def host_prove_rep3_party(session, pub, wit_a, wit_b, net_table, rand_table, streams_table=None):
    """ONE REP3 party on an open ProvingSession through the callback ABI; returns (proof, seconds).  Call it from one thread per party.
    streams_table (Rep3ChaChaTable): the masking vectors are drawn on the GPU from the described ChaCha12 generators."""
    nq = 6 if session.curve == BLS12_381 else 4
    out = np.zeros(8 * nq, dtype=np.uint64); sec = (C.c_double * 1)()
    keep = [np.ascontiguousarray(x, dtype=np.uint64) for x in (pub, wit_a, wit_b)]
    _hchk(load_host().cgh_session_prove_rep3_party_ex(session.h, _hp(keep[0]), _hp(keep[1]), _hp(keep[2]), C.byref(net_table), C.byref(rand_table),
                                                      C.byref(streams_table) if streams_table is not None else None, _hp(out), sec))
    return out, sec[0]


def host_plonk_zkey_info(curve, path):
    info = (C.c_size_t * 6)()
    _hchk(load_host().cgh_plonk_zkey_info(curve, path.encode(), info))
    return dict(zip(("n_vars", "n_public", "domain_size", "power", "n_additions", "n_constraints"), [int(x) for x in info]))


PLONK_COMMITS = ("a", "b", "c", "z", "t1", "t2", "t3", "wxi", "wxiw")
PLONK_CHALLENGES = ("beta", "gamma", "alpha", "xi", "v")
PLONK_EVALS = ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw")


def _pad_blind(blind):
    blind = np.ascontiguousarray(blind, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros((11, 4), dtype=np.uint64); out[:blind.shape[0]] = blind
    return out


def plonk_prove_plain(curve, zkey_path, full_witness, blind, upto=5, device=0, want_t=False, want_poly_z=False):
    """co-plonk with the plain driver on the GPU through round `upto` (<= 5): dict of commitments, challenges, evaluations[, t polys, poly_z]
    (the proof of co-plonk/src/plonk.rs = the nine commitments and six evaluations)"""
    info = host_plonk_zkey_info(curve, zkey_path)
    nq = 6 if curve == BLS12_381 else 4; n = info["domain_size"]
    commits = np.zeros((9, 2 * nq), dtype=np.uint64); ch = np.zeros((5, 4), dtype=np.uint64); ev = np.zeros((6, 4), dtype=np.uint64)
    tp = np.zeros((3 * n + 8, 4), dtype=np.uint64) if want_t else None
    pz = np.zeros((n + 3, 4), dtype=np.uint64) if want_poly_z else None
    _hchk(load_host().cgh_plonk_prove_plain(int(device), curve, zkey_path.encode(), _hp(np.ascontiguousarray(full_witness, dtype=np.uint64)),
                                            _hp(_pad_blind(blind)), int(upto), _hp(commits), _hp(ch), _hp(ev), _hp(tp) if want_t else None, _hp(pz) if want_poly_z else None))
    out = dict(zip(PLONK_COMMITS, commits)); out.update(zip(PLONK_CHALLENGES, ch)); out.update(zip(PLONK_EVALS, ev))
    if want_t: out.update(t1_poly=tp[:n + 1], t2_poly=tp[n + 1:2 * n + 2], t3_poly=tp[2 * n + 2:])
    if want_poly_z: out["poly_z"] = pz
    return out


def plonk_round1_plain(curve, zkey_path, full_witness, blind, device=0):
    """the three wire commitments (3, packed G1)"""
    r = plonk_prove_plain(curve, zkey_path, full_witness, blind, upto=1, device=device)
    return np.stack([r["a"], r["b"], r["c"]])


def plonk_round2_plain(curve, zkey_path, full_witness, blind, device=0, want_poly=False):
    """rounds 1 + 2: (beta, gamma, commit_z[, poly_z])"""
    r = plonk_prove_plain(curve, zkey_path, full_witness, blind, upto=2, device=device, want_poly_z=want_poly)
    return (r["beta"], r["gamma"], r["z"], r["poly_z"]) if want_poly else (r["beta"], r["gamma"], r["z"])


def plonk_prove_rep3(curve, zkey_path, pub, wit_a, wit_b, blind_a, blind_b, streams=None, upto=5, device=0):
    """three REP3 parties (threads) on one GPU through round `upto`; returns a list of three dicts (one per party) like plonk_prove_plain"""
    nq = 6 if curve == BLS12_381 else 4
    commits = np.zeros((3, 9, 2 * nq), dtype=np.uint64); ch = np.zeros((3, 5, 4), dtype=np.uint64); ev = np.zeros((3, 6, 4), dtype=np.uint64)
    lists = [wit_a, wit_b, [_pad_blind(x) for x in blind_a], [_pad_blind(x) for x in blind_b]] + ([streams] if streams is not None else [])
    keep = [[np.ascontiguousarray(x, dtype=np.uint64) for x in lst] for lst in lists]
    arr = lambda lst: (C.c_void_p * 3)(*[x.ctypes.data for x in lst])
    _hchk(load_host().cgh_plonk_prove_rep3(int(device), curve, zkey_path.encode(), _hp(np.ascontiguousarray(pub, dtype=np.uint64)), arr(keep[0]), arr(keep[1]),
                                           arr(keep[2]), arr(keep[3]), arr(keep[4]) if streams is not None else None,
                                           C.c_size_t(keep[4][0].shape[0] if streams is not None else 0), int(upto), _hp(commits), _hp(ev), _hp(ch)))
    out = []
    for i in range(3):
        dct = dict(zip(PLONK_COMMITS, commits[i])); dct.update(zip(PLONK_CHALLENGES, ch[i])); dct.update(zip(PLONK_EVALS, ev[i]))
        out.append(dct)
    return out


def plonk_prove_rep3_party(curve, zkey_path, pub, wit_a, wit_b, net_table, rand_table, blind_a=None, blind_b=None, upto=5, device=0, streams_table=None):
    """ONE REP3 party of co-plonk through the callback ABI (cgh_plonk_prove_rep3_party); blind_a/blind_b None = drawn with rand() first.
    Returns a dict like plonk_prove_plain.  Call it from one thread per party."""
    nq = 6 if curve == BLS12_381 else 4
    commits = np.zeros((9, 2 * nq), dtype=np.uint64); ch = np.zeros((5, 4), dtype=np.uint64); ev = np.zeros((6, 4), dtype=np.uint64)
    keep = [np.ascontiguousarray(x, dtype=np.uint64) for x in (pub, wit_a, wit_b)]
    bl = [None if x is None else _pad_blind(x) for x in (blind_a, blind_b)]
    _hchk(load_host().cgh_plonk_prove_rep3_party_ex(int(device), curve, zkey_path.encode(), _hp(keep[0]), _hp(keep[1]), _hp(keep[2]),
                                                    None if bl[0] is None else _hp(bl[0]), None if bl[1] is None else _hp(bl[1]),
                                                    C.byref(net_table), C.byref(rand_table), C.byref(streams_table) if streams_table is not None else None,
                                                    int(upto), _hp(commits), _hp(ev), _hp(ch)))
    dct = dict(zip(PLONK_COMMITS, commits)); dct.update(zip(PLONK_CHALLENGES, ch)); dct.update(zip(PLONK_EVALS, ev))
    return dct


def _shamir_extras(timing):
    return ((C.c_double * 6)() if timing else None), (C.c_size_t * 4)()


def _shamir_stats(rs, ps):
    st = dict(zip(("pairs_consumed", "pairs_left", "lazy_batches", "pairs_from_device"), [int(x) for x in ps]))
    st["round_seconds"] = None if rs is None else [float(x) for x in rs]
    return st


def plonk_prove_shamir_party(curve, zkey_path, threshold, pub, wit, net_table, rand_table, blind=None, preprocess=0, upto=5, device=0, timing=False):
    """ONE Shamir party of co-plonk through the callback ABI (cgh_plonk_prove_shamir_party); blind None = drawn with rand() first.
    Returns (proof dict, seconds, stats): stats = pairs_consumed / pairs_left / lazy_batches / pairs_from_device and, with timing=True,
    round_seconds = [preprocessing, round 1 .. round 5].  Call it from one thread per party."""
    nq = 6 if curve == BLS12_381 else 4
    commits = np.zeros((9, 2 * nq), dtype=np.uint64); ch = np.zeros((5, 4), dtype=np.uint64); ev = np.zeros((6, 4), dtype=np.uint64)
    keep = [np.ascontiguousarray(x, dtype=np.uint64) for x in (pub, wit)]
    bl = None if blind is None else _pad_blind(blind)
    sec = (C.c_double * 1)(); rs, ps = _shamir_extras(timing)
    _hchk(load_host().cgh_plonk_prove_shamir_party(int(device), curve, zkey_path.encode(), int(threshold), _hp(keep[0]), _hp(keep[1]), _hp(bl),
                                                   C.byref(net_table), C.byref(rand_table), C.c_size_t(int(preprocess)), int(upto),
                                                   _hp(commits), _hp(ev), _hp(ch), sec, rs, ps))
    dct = dict(zip(PLONK_COMMITS, commits)); dct.update(zip(PLONK_CHALLENGES, ch)); dct.update(zip(PLONK_EVALS, ev))
    return dct, sec[0], _shamir_stats(rs, ps)


def _plonk_proof_arrays(curve, proofs):
    """(commits (n, 9, point words), evals (n, 6, 4)) of a list of proof dicts, or of a (commits, evals) pair of stacked arrays"""
    nq = fq_limbs(curve)
    if isinstance(proofs, tuple):
        commits, evals = proofs
    else:
        proofs = list(proofs)
        commits = np.stack([np.stack([p[k] for k in PLONK_COMMITS]) for p in proofs]) if proofs else np.zeros((0, 9, 2 * nq), dtype=np.uint64)
        evals = np.stack([np.stack([p[k] for k in PLONK_EVALS]) for p in proofs]) if proofs else np.zeros((0, 6, 4), dtype=np.uint64)
    commits = np.ascontiguousarray(commits, dtype=np.uint64).reshape(-1, 9, 2 * nq)
    return commits, np.ascontiguousarray(evals, dtype=np.uint64).reshape(commits.shape[0], 6, 4)


class PlonkVerifyingKey:
    """Plonk verifying key (cgh_plonk_vk_*): points validated, the domain's root of unity checked against the library's own when the handle is opened"""
    POINTS = ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")

    def __init__(self, curve, handle):
        self.curve, self.h = curve, handle
        info = (C.c_size_t * 3)()
        _hchk(load_host().cgh_plonk_vk_info(self.h, info))
        self.n_public, self.power = int(info[1]), int(info[2])

    @classmethod
    def from_json(cls, curve, path):
        h = C.c_void_p()
        _hchk(load_host().cgh_plonk_vk_from_json(curve, path.encode(), C.byref(h)))
        return cls(curve, h)

    @classmethod
    def from_zkey(cls, curve, path):
        h = C.c_void_p()
        _hchk(load_host().cgh_plonk_vk_from_zkey(curve, path.encode(), C.byref(h)))
        return cls(curve, h)

    def close(self):
        if self.h: load_host().cgh_plonk_vk_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fields(self):
        """dict of the key's fields: Qm .. S3, X_2 (packed affine, Montgomery), k1, k2, w, nPublic, power"""
        nq = fq_limbs(self.curve)
        out = np.zeros(20 * nq + 12, dtype=np.uint64)
        _hchk(load_host().cgh_plonk_vk_fields(self.h, _hp(out)))
        d = dict(zip(self.POINTS, out[:16 * nq].reshape(8, 2 * nq)))
        d.update(X_2=out[16 * nq:20 * nq], k1=out[20 * nq:20 * nq + 4], k2=out[20 * nq + 4:20 * nq + 8], w=out[20 * nq + 8:], nPublic=self.n_public, power=self.power)
        return d

    def scalars_key(self):
        """the key as plonk_verify_scalars_host / Context.plonk_verify_scalars take it"""
        f = self.fields()
        return dict(points=np.stack([f[k] for k in self.POINTS]), k1=f["k1"], k2=f["k2"], omega=f["w"], power=self.power)

    def verify(self, proof, pub):
        """one proof (the dict the prove entries return) on the host (cgh_plonk_verify); a wrong number of public inputs or a non-canonical one raises BackendError"""
        commits, evals = _plonk_proof_arrays(self.curve, [proof])
        pub = np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 4)
        ok = C.c_int32(0)
        _hchk(load_host().cgh_plonk_verify(self.h, _hp(commits), _hp(evals), _hp(pub), C.c_size_t(pub.shape[0]), C.byref(ok)))
        return bool(ok.value)

    def verify_batch(self, proofs, pubs, seed=None, per_proof=False, device=0, timing=False):
        """n proofs on the GPU with random 128-bit coefficients (cgh_plonk_verify_batch).  proofs: a list of proof dicts or a (commits, evals)
        pair of stacked arrays; pubs: (n, n_public, 4).  Returns the verdict; with per_proof=True (verdict, flags); with timing=True the
        five stage times in seconds are appended."""
        commits, evals = _plonk_proof_arrays(self.curve, proofs)
        n = commits.shape[0]
        pubs = np.ascontiguousarray(pubs, dtype=np.uint64).reshape(n, self.n_public, 4) if n else np.zeros((0, self.n_public, 4), dtype=np.uint64)
        ok = C.c_int32(0)
        flags = np.zeros(max(n, 1), dtype=np.uint8) if per_proof else None
        secs = (C.c_double * 5)()
        _hchk(load_host().cgh_plonk_verify_batch_timed(int(device), self.h, _hp(commits), _hp(evals), _hp(pubs), C.c_size_t(pubs.shape[1]), C.c_size_t(n),
                                                       None if seed is None else bytes(seed), C.byref(ok), _hp(flags), secs))
        out = (bool(ok.value),) + ((flags[:n].astype(bool),) if per_proof else ()) + ((list(secs),) if timing else ())
        return out[0] if len(out) == 1 else out


class PlonkSession:
    """co-plonk proving session (cgh_plonk_session_*): the zkey is read once; p_tau (validated, with per-window tables), the q / sigma /
    Lagrange polynomials, the wire maps and the additions' level schedule stay on the device; proofs (rounds 1..5) read them there"""

    def __init__(self, curve, zkey_path, precompute=True, device=0, validate=True):
        self.curve, self.h = curve, None
        h = C.c_void_p()
        _hchk(load_host().cgh_plonk_session_open(int(device), curve, zkey_path.encode(), -1 if precompute is True else int(precompute),
                                                 C.c_uint32(0 if validate else 1), C.byref(h)))
        self.h = h
        info = (C.c_size_t * 6)()
        _hchk(load_host().cgh_plonk_session_info(self.h, info))
        self.info = dict(zip(("n_vars", "n_public", "domain_size", "power", "n_additions", "n_constraints"), [int(x) for x in info]))

    def close(self):
        if self.h: load_host().cgh_plonk_session_close(self.h); self.h = None

    def _outputs(self):
        nq = 6 if self.curve == BLS12_381 else 4
        return np.zeros((9, 2 * nq), dtype=np.uint64), np.zeros((6, 4), dtype=np.uint64), np.zeros((5, 4), dtype=np.uint64), (C.c_double * 1)()

    def _rows(self, name, x, n):
        x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)
        if x.shape[0] != n:
            raise BackendError(f"PlonkSession: {name} has {x.shape[0]} elements, the zkey wants {n}")
        return x

    def prove_plain(self, full_witness, blind):
        """full_witness = n_vars - n_additions elements (leading one, public inputs, private witness); returns (proof dict, seconds)"""
        i = self.info
        w = self._rows("full_witness", full_witness, i["n_vars"] - i["n_additions"])
        commits, ev, ch, sec = self._outputs()
        _hchk(load_host().cgh_plonk_session_prove_plain(self.h, _hp(w), _hp(_pad_blind(blind)), _hp(commits), _hp(ev), _hp(ch), sec))
        dct = dict(zip(PLONK_COMMITS, commits)); dct.update(zip(PLONK_CHALLENGES, ch)); dct.update(zip(PLONK_EVALS, ev))
        return dct, sec[0]

    def verify(self, proof, pub):
        """Plonk::verify of a proof (the dict the prove entries return) against the session's own key (cgh_plonk_session_verify); pub = the
        n_public public inputs, Montgomery"""
        commits, evals = _plonk_proof_arrays(self.curve, [proof])
        pub = self._rows("pub", pub, self.info["n_public"])
        ok = C.c_int32(0)
        _hchk(load_host().cgh_plonk_session_verify(self.h, _hp(commits), _hp(evals), _hp(pub), C.byref(ok)))
        return bool(ok.value)

    def check_witness(self, full_witness):
        """(n_bad, first_bad) of the plain full witness against every row of the key (cgh_plonk_session_check_witness): the number of gate
        rows it breaks and the smallest one, NO_ROW when it satisfies the key.  No proof is made."""
        i = self.info
        w = self._rows("full_witness", full_witness, i["n_vars"] - i["n_additions"])
        n_bad, first = C.c_uint64(0), C.c_uint64(0)
        _hchk(load_host().cgh_plonk_session_check_witness(self.h, _hp(w), C.byref(n_bad), C.byref(first)))
        return int(n_bad.value), int(first.value)

    def audit(self, r1cs=None, seed=None, timing=False):
        """is the key what `plonk setup` writes (cgh_plonk_session_audit)?  -> (failed, detail): failed = PLONK_AUDIT_* bits, detail = one
        (which, index) pair per check in the order of PLONK_AUDIT_NAMES, (None, None) for a check that passed.  r1cs: an R1cs to audit the
        key against its circuit as well; seed: 32 bytes for the SRS check's coefficients (None = OS entropy).  timing=True: also the
        seconds of PLONK_AUDIT_STAGES"""
        failed = C.c_uint32(0)
        det = (C.c_uint64 * (2 * len(PLONK_AUDIT_NAMES)))()
        sec = (C.c_double * len(PLONK_AUDIT_STAGES))()
        sd = None if seed is None else (C.c_uint8 * 32).from_buffer_copy(bytes(seed))
        _hchk(load_host().cgh_plonk_session_audit_timed(self.h, None if r1cs is None else r1cs.h, sd, C.byref(failed), det, sec))
        opt = lambda v: None if v == NO_ROW else int(v)
        detail = [(opt(det[2 * k]), opt(det[2 * k + 1])) for k in range(len(PLONK_AUDIT_NAMES))]
        return (int(failed.value), detail, dict(zip(PLONK_AUDIT_STAGES, sec))) if timing else (int(failed.value), detail)

    def prove_rep3_party(self, pub, wit_a, wit_b, net_table, rand_table, blind_a=None, blind_b=None, streams_table=None):
        """ONE REP3 party through the callback ABI (cgh_plonk_session_prove_rep3_party); blind_a/blind_b None = drawn with rand() first.
        Returns (proof dict, seconds).  Call it from one thread per party, each on its own session."""
        i = self.info
        n_priv = i["n_vars"] - i["n_additions"] - i["n_public"] - 1
        keep = [self._rows("pub", pub, i["n_public"] + 1), self._rows("wit_a", wit_a, n_priv), self._rows("wit_b", wit_b, n_priv)]
        bl = [None if x is None else _pad_blind(x) for x in (blind_a, blind_b)]
        commits, ev, ch, sec = self._outputs()
        _hchk(load_host().cgh_plonk_session_prove_rep3_party(self.h, _hp(keep[0]), _hp(keep[1]), _hp(keep[2]),
                                                             None if bl[0] is None else _hp(bl[0]), None if bl[1] is None else _hp(bl[1]),
                                                             C.byref(net_table), C.byref(rand_table),
                                                             C.byref(streams_table) if streams_table is not None else None,
                                                             _hp(commits), _hp(ev), _hp(ch), sec))
        dct = dict(zip(PLONK_COMMITS, commits)); dct.update(zip(PLONK_CHALLENGES, ch)); dct.update(zip(PLONK_EVALS, ev))
        return dct, sec[0]


    def shamir_pairs(self, threshold, with_blinding=False):
        """double-sharing pairs ONE Shamir proof on this session consumes (cgh_plonk_session_shamir_pairs); preprocess = ceil(pairs / (t + 1))"""
        out = C.c_size_t()
        _hchk(load_host().cgh_plonk_session_shamir_pairs(self.h, int(threshold), int(bool(with_blinding)), C.byref(out)))
        return int(out.value)

    def _shamir_party(self, threshold, pub, wit, net_table, rand_table, seed, blind, preprocess, timing):
        i = self.info
        keep = [self._rows("pub", pub, i["n_public"] + 1), self._rows("wit", wit, i["n_vars"] - i["n_additions"] - i["n_public"] - 1)]
        bl = None if blind is None else _pad_blind(blind)
        commits, ev, ch, sec = self._outputs()
        rs, ps = _shamir_extras(timing)
        if seed is None:
            _hchk(load_host().cgh_plonk_session_prove_shamir_party(self.h, int(threshold), _hp(keep[0]), _hp(keep[1]), _hp(bl), C.byref(net_table), C.byref(rand_table),
                                                                   C.c_size_t(int(preprocess)), _hp(commits), _hp(ev), _hp(ch), sec, rs, ps))
        else:
            seed = bytes(seed)
            if len(seed) != 32:
                raise BackendError("PlonkSession: the seed is 32 bytes")
            _hchk(load_host().cgh_plonk_session_prove_shamir_party_seeded(self.h, int(threshold), _hp(keep[0]), _hp(keep[1]), _hp(bl), C.byref(net_table), seed,
                                                                          C.c_size_t(int(preprocess)), _hp(commits), _hp(ev), _hp(ch), sec, rs, ps))
        dct = dict(zip(PLONK_COMMITS, commits)); dct.update(zip(PLONK_CHALLENGES, ch)); dct.update(zip(PLONK_EVALS, ev))
        return dct, sec[0], _shamir_stats(rs, ps)

    def prove_shamir_party(self, threshold, pub, wit, net_table, rand_table, blind=None, preprocess=0, timing=False):
        """ONE Shamir party (threshold t of net_table.num_parties) through the callback ABI (cgh_plonk_session_prove_shamir_party); blind None =
        drawn with rand() first.  Returns (proof dict, seconds, stats) like plonk_prove_shamir_party.  One thread per party, each on its own session."""
        return self._shamir_party(threshold, pub, wit, net_table, rand_table, None, blind, preprocess, timing)

    def prove_shamir_party_seeded(self, threshold, pub, wit, net_table, seed, blind=None, preprocess=0, timing=False):
        """the same party with its private randomness as one 32-byte seed of the library's ChaCha12 stream (large draws on the GPU)"""
        return self._shamir_party(threshold, pub, wit, net_table, None, seed, blind, preprocess, timing)


def plonk_prove_shamir(curve, zkey_path, n, t, pub, wits, blinds, streams, upto=5, device=0):
    """n Shamir parties (threshold t) on one GPU through round `upto`; returns a list of n dicts like plonk_prove_plain"""
    nq = 6 if curve == BLS12_381 else 4
    commits = np.zeros((n, 9, 2 * nq), dtype=np.uint64); ch = np.zeros((n, 5, 4), dtype=np.uint64); ev = np.zeros((n, 6, 4), dtype=np.uint64)
    keep = [[np.ascontiguousarray(x, dtype=np.uint64) for x in lst] for lst in (wits, [_pad_blind(x) for x in blinds], streams)]
    arr = lambda lst: (C.c_void_p * n)(*[x.ctypes.data for x in lst])
    _hchk(load_host().cgh_plonk_prove_shamir(int(device), curve, zkey_path.encode(), int(n), int(t), _hp(np.ascontiguousarray(pub, dtype=np.uint64)),
                                             arr(keep[0]), arr(keep[1]), arr(keep[2]), C.c_size_t(keep[2][0].shape[0]), int(upto), _hp(commits), _hp(ev), _hp(ch)))
    out = []
    for i in range(n):
        dct = dict(zip(PLONK_COMMITS, commits[i])); dct.update(zip(PLONK_CHALLENGES, ch[i])); dct.update(zip(PLONK_EVALS, ev[i]))
        out.append(dct)
    return out


def plonk_round1_rep3(curve, zkey_path, pub, wit_a, wit_b, blind_a, blind_b, device=0):
    """round 1 only: (3 parties, 3 commitments, packed G1)"""
    r = plonk_prove_rep3(curve, zkey_path, pub, wit_a, wit_b, blind_a, blind_b, streams=None, upto=1, device=device)
    return np.stack([np.stack([p["a"], p["b"], p["c"]]) for p in r])


def host_shared_witness_write(curve, path, pub, a, b=None):
    """`.shared` witness file (bincode + ark-compressed vectors): REP3 when b is given, Shamir otherwise.  Layout restated from the
    reference's types; the snapshot holds no .shared fixture to pin it against."""
    pub = np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 4); a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    _hchk(load_host().cgh_shared_witness_write(curve, path.encode(), 0 if b is not None else 1, _hp(pub), C.c_size_t(pub.shape[0]), _hp(a), _hp(bb), C.c_size_t(a.shape[0])))


def host_shared_witness_read(curve, path, rep3=True):
    sizes = (C.c_size_t * 2)()
    _hchk(load_host().cgh_shared_witness_read(curve, path.encode(), 0 if rep3 else 1, sizes, None, None, None))
    pub = np.zeros((sizes[0], 4), dtype=np.uint64); a = np.zeros((sizes[1], 4), dtype=np.uint64); b = np.zeros((sizes[1], 4), dtype=np.uint64) if rep3 else None
    _hchk(load_host().cgh_shared_witness_read(curve, path.encode(), 0 if rep3 else 1, sizes, _hp(pub), _hp(a), _hp(b)))
    return (pub, a, b) if rep3 else (pub, a)


def host_plonk_proof_to_json(curve, proof):
    """PlonkProof JSON text (circom-types/src/plonk/proof.rs) of a proof dict (PLONK_COMMITS + PLONK_EVALS keys)"""
    commits = np.ascontiguousarray(np.stack([proof[k] for k in PLONK_COMMITS]), dtype=np.uint64)
    evals = np.ascontiguousarray(np.stack([proof[k] for k in PLONK_EVALS]), dtype=np.uint64)
    buf = C.create_string_buffer(8192)
    _hchk(load_host().cgh_plonk_proof_to_json(curve, _hp(commits), _hp(evals), buf, C.c_size_t(8192)))
    return buf.value.decode()


def host_plonk_proof_from_json(curve, text):
    nq = 6 if curve == BLS12_381 else 4
    commits = np.zeros((9, 2 * nq), dtype=np.uint64); evals = np.zeros((6, 4), dtype=np.uint64)
    _hchk(load_host().cgh_plonk_proof_from_json(curve, text.encode(), _hp(commits), _hp(evals)))
    out = dict(zip(PLONK_COMMITS, commits)); out.update(zip(PLONK_EVALS, evals))
    return out


def host_plonk_transcript(curve, items):
    """items: list of ("scalar", limbs) / ("point", packed G1 limbs) -> challenge computed by the host mirror's Keccak256 transcript"""
    n = len(items)
    kinds = (C.c_int32 * n)(*[0 if k == "scalar" else 1 for k, _ in items])
    keep = [np.ascontiguousarray(v, dtype=np.uint64) for _, v in items]
    ptrs = (C.c_void_p * n)(*[v.ctypes.data for v in keep])
    out = np.zeros(4, dtype=np.uint64)
    _hchk(load_host().cgh_plonk_transcript(curve, kinds, ptrs, n, _hp(out)))
    return out


def host_read_wtns(curve, path):
    n = C.c_size_t(0)
    _hchk(load_host().cgh_read_wtns(curve, path.encode(), None, C.c_size_t(0), C.byref(n)))
    out = np.zeros((n.value, 4), dtype=np.uint64)
    _hchk(load_host().cgh_read_wtns(curve, path.encode(), _hp(out), C.c_size_t(n.value), C.byref(n)))
    return out


def prove_plain(curve, zkey_path, full_witness, r, s, device=0, want_h=False):
    """PlainHipDriver + CoGroth16::prove; returns packed proof A||B||C (and the h vector)"""
    info = host_zkey_info(curve, zkey_path)
    w = np.ascontiguousarray(full_witness, dtype=np.uint64)
    out = np.zeros(8 * fq_limbs(curve), dtype=np.uint64)
    h = np.zeros((info["domain_size"], 4), dtype=np.uint64) if want_h else None
    _hchk(load_host().cgh_prove_plain(int(device), curve, zkey_path.encode(), _hp(w), _hp(np.ascontiguousarray(r, dtype=np.uint64)),
                                      _hp(np.ascontiguousarray(s, dtype=np.uint64)), _hp(out), _hp(h)))
    return (out, h) if want_h else out


def prove_rep3(curve, zkey_path, pub, wit_a, wit_b, streams, device=0, want_h=False):
    """three Rep3HipProtocol parties on three threads over the in-process network; returns the three proofs"""
    info = host_zkey_info(curve, zkey_path)
    pub = np.ascontiguousarray(pub, dtype=np.uint64)
    wa = [np.ascontiguousarray(x, dtype=np.uint64) for x in wit_a]
    wb = [np.ascontiguousarray(x, dtype=np.uint64) for x in wit_b]
    st = [np.ascontiguousarray(x, dtype=np.uint64) for x in streams]
    arr = lambda xs: (C.c_void_p * 3)(*[x.ctypes.data for x in xs])
    out = np.zeros((3, 8 * fq_limbs(curve)), dtype=np.uint64)
    h = np.zeros((2, info["domain_size"], 4), dtype=np.uint64) if want_h else None
    _hchk(load_host().cgh_prove_rep3(int(device), curve, zkey_path.encode(), _hp(pub), arr(wa), arr(wb), arr(st), C.c_size_t(st[0].shape[0]), _hp(out), _hp(h)))
    return (out, h) if want_h else out
