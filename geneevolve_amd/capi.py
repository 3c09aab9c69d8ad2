"""ctypes binding of the C-ABI declared in include/geneevolve_amd.h.

This is the stub a Python host would add; the C++ host binding is shown in INTEGRATION.md.
`GevLibrary(path, prefix)` binds any shared library that exports the ABI under `prefix`
(the product library exports `gev_*`).  No compute happens in Python: every method is one
C call on caller-owned numpy buffers.  Every function is typed from one table, `ABI`, which
tests/test_abi_cpu.py holds equal to the header: a new entry point adds a line there and a method.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.environ.get("GEV_LIBRARY_PATH") or os.path.join(_HERE, "csrc", "libgeneevolve_amd.so")   # (the variable: A/B builds of the same library)


class GevError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class gev_couple(C.Structure):
    _fields_ = [("pos_male", C.c_uint64), ("pos_female", C.c_uint64), ("inbreed", C.c_int32), ("num_offspring", C.c_int32)]


class gev_part(C.Structure):
    _fields_ = [("st", C.c_uint64), ("en", C.c_uint64), ("hap_index", C.c_uint64), ("root_population", C.c_int32), ("reserved", C.c_int32)]


class gev_ibd_segment(C.Structure):
    _fields_ = [("st", C.c_uint64), ("en", C.c_uint64), ("row_a", C.c_uint32), ("row_b", C.c_uint32)]


class gev_lineage_site(C.Structure):
    _fields_ = [("sum_sq", C.c_uint64), ("n_covered", C.c_uint32), ("n_lineages", C.c_uint32), ("top_count", C.c_uint32), ("top_founder", C.c_uint32)]


class gev_roh_params(C.Structure):
    _fields_ = [("min_snps", C.c_uint32), ("reserved", C.c_uint32), ("min_bp", C.c_uint64), ("max_gap_bp", C.c_uint64)]


class gev_roh_segment(C.Structure):
    _fields_ = [("st", C.c_uint64), ("en", C.c_uint64), ("ind", C.c_uint32), ("snp_first", C.c_uint32), ("n_snps", C.c_uint32), ("reserved", C.c_uint32)]


class gev_move(C.Structure):
    _fields_ = [("src_pop", C.c_int32), ("dst_pop", C.c_int32), ("src_pos", C.c_uint64)]


class gev_gef_params(C.Structure):
    _fields_ = [("va", C.c_double), ("vd", C.c_double), ("ve", C.c_double), ("vf", C.c_double), ("beta", C.c_double),
                ("s2_a_gen0", C.c_double), ("s2_d_gen0", C.c_double), ("gen_num", C.c_int32), ("reserved", C.c_int32)]


class gev_pheno_scheme(C.Structure):
    _fields_ = [("va", C.c_double), ("vd", C.c_double), ("vc", C.c_double), ("ve", C.c_double), ("vf", C.c_double), ("beta", C.c_double)]


class gev_phenotypes_params(C.Structure):
    _fields_ = [("gen_num", C.c_int32), ("vt_type", C.c_int32), ("scheme", C.c_void_p)]


PHENOTYPE_COMPONENTS = ("additive", "dominance", "bv", "common_sibling", "e_noise", "parental_effect", "phen")


class gev_selection_params(C.Structure):
    _fields_ = [("gen_num", C.c_int32), ("func", C.c_int32), ("par1", C.c_double), ("par2", C.c_double),
                ("omega", C.c_void_p), ("lambda_", C.c_void_p), ("phen_shift", C.c_void_p)]


# GEV_SEL_* of include/geneevolve_amd.h by the reference's names of the functions (Population::_selection_func; "" = logit 0 1)
SELECTION_FUNCS = {"none": 0, "": 1, "logit": 2, "probit": 3, "stab": 4, "thr": 5}


class gev_generation_result(C.Structure):
    _fields_ = [("glob_state", C.c_uint32), ("seed_mate", C.c_uint32), ("seed_reproduce", C.c_uint32), ("reserved", C.c_uint32),
                ("num_males_mate", C.c_uint64), ("num_females_mate", C.c_uint64)]


class gev_assort_params(C.Structure):
    _fields_ = [("pop_size", C.c_uint64), ("mat_cor", C.c_double), ("mm_percent", C.c_double), ("avoid_inbreeding", C.c_int32),
                ("offspring_dist", C.c_int32)]


class gev_assort_result(C.Structure):
    _fields_ = [("num_males_mate", C.c_uint64), ("num_females_mate", C.c_uint64), ("n_couples", C.c_uint64), ("n_inbreed", C.c_uint64),
                ("n_offspring", C.c_uint64)]


def _assort_result(r):
    return {k: int(getattr(r, k)) for k, _ in gev_assort_result._fields_}


COUPLE_DTYPE = np.dtype(gev_couple)
PART_DTYPE = np.dtype(gev_part)
MOVE_DTYPE = np.dtype(gev_move)
SEGMENT_DTYPE = np.dtype(gev_ibd_segment)       # 24 bytes: st, en (uint64, [st, en)), row_a, row_b (uint32)
IBD_ALL_PAIRS, IBD_UPPER = 0, 1
LINEAGE_SITE_DTYPE = np.dtype(gev_lineage_site)  # 24 bytes: sum_sq (uint64), n_covered, n_lineages, top_count, top_founder (uint32)
NO_FOUNDER = 0xFFFFFFFF                          # GEV_NO_FOUNDER: the founder id of a position no part covers
ROH_PARAMS_DTYPE = np.dtype(gev_roh_params)      # 24 bytes: min_snps, reserved (uint32), min_bp, max_gap_bp (uint64); 0 = no limit, each
ROH_SEGMENT_DTYPE = np.dtype(gev_roh_segment)    # 32 bytes: st, en (uint64, both inclusive), ind, snp_first, n_snps, reserved (uint32)

# Every function include/geneevolve_amd.h declares, in its order, as "return: parameters" (tests hold the table equal to the header
# and check that the library exports every name).  By value: int, size (size_t), u32, u64, f64.  `ctx*` is the context handle.  A
# pointer is its element and a star: int i32 u32 i64 u64 ull (unsigned long long) size f32 f64, u8 (char and uint8_t alike), void, or a
# gev_* struct by its name without the prefix; two stars: a pointer to pointers.  Returns: int, u32, void, f64, str (const char*).
ABI = {
    "last_error": "str:",
    "version": "str:",
    "create": "int: ctx** int int int int",
    "destroy": "void: ctx*",
    "set_rmap": "int: ctx* int int u64* f64* size u64",
    "set_mutmap": "int: ctx* int int u64* f64* size",
    "set_snps": "int: ctx* int int u64* size",
    "set_cvs": "int: ctx* int int int u64* f64* f64* size f64",
    "upload_founders": "int: ctx* int int u64* size size size",
    "upload_cv_founders": "int: ctx* int int int u64* size size size",
    "synth_founders": "int: ctx* int int size u64",
    "synth_cv_founders": "int: ctx* int int int size u64",
    "init_gen0": "int: ctx* int size u32 u8*",
    "reproduce": "int: ctx* int couple* size u32 u32* size size u8*",
    "presample": "int: ctx* int u32 u32* size size",
    "reproduce_begin": "int: ctx* int couple* size u32 u32* size size",
    "reproduce_end": "int: ctx* u8*",
    "presample_sex": "int: ctx* int u8* size",
    "random_mate": "int: ctx* int u32 f64* size couple* size* size*",
    "glob_seeds": "int: ctx* u32* size u32*",
    "generation_begin": "int: ctx* int u32 size f64*",
    "generation_end": "int: ctx* generation_result* couple* u8*",
    "set_generation_chain": "int: ctx* int",
    "compute_ad": "int: ctx* int f64* f64* f64* f64*",
    "scale_ad_compute_gef": "int: ctx* int int gef_params* u32 f64* f64* f64* f64* f64* f64* f64* f64* f64*",
    "compute_selection": "int: ctx* int selection_params* f64* f64* f64*",
    "download_selection": "int: ctx* int f64* f64* f64*",
    "get_selection_gen0": "int: ctx* int f64* f64*",
    "set_selection_gen0": "int: ctx* int f64 f64",
    "generation_begin_selected": "int: ctx* int u32 size",
    "random_mate_selected": "int: ctx* int u32 size couple* size* size*",
    "set_track_pedigree": "int: ctx* int",
    "download_pedigree": "int: ctx* int i64*",
    "upload_pedigree": "int: ctx* int i64*",
    "generation_phenotypes": "int: ctx* int phenotypes_params* u32",
    "phenotypes_result": "int: ctx* int u32* u32* f64*",
    "download_phenotypes": "int: ctx* int int f64*",
    "get_ad_gen0": "int: ctx* int int f64* f64*",
    "set_ad_gen0": "int: ctx* int int f64 f64",
    "save_prev_gen": "int: ctx* int f64*",
    "upload_prev_gen": "int: ctx* int f64* f64* size",
    "dbg_phenotype_knobs": "int: ctx* int ull*",
    "format_info_text": "int: ctx* int size size int u8* size size*",
    "dbg_format_g": "int: ctx* f64* size u8* ull*",
    "dbg_format_g_host": "int: f64* size u8* ull*",
    "set_founder_names": "int: ctx* int u8* u32* size",
    "format_interval_text": "int: ctx* int int int size size int i64* u8* size size*",
    "dbg_format_interval_text_host": "int: part* u64* size i64* int u8** u32** size* int int u8* size size*",
    "assort_mate": "int: ctx* int assort_params* u32* f64* f64* i64* couple* assort_result*",
    "assort_mate_selected": "int: ctx* int assort_params* u32* i64* couple* assort_result*",
    "last_assort_result": "int: ctx* assort_result* couple*",
    "generation_begin_assort": "int: ctx* int u32 assort_params* f64* f64* i64*",
    "generation_begin_assort_selected": "int: ctx* int u32 assort_params* i64*",
    "dbg_assort_knobs": "int: ctx* int int",
    "dbg_assort_stats": "int: ctx* ull*",
    "set_ad": "int: ctx* int f64* f64*",
    "get_cv_freq": "int: ctx* int int int f64* size",
    "migrate": "int: ctx* move* size",
    "export_size": "int: ctx* int u64* size size*",
    "export_rows": "int: ctx* int u64* size void* size",
    "remove_rows": "int: ctx* int u64* size",
    "import_rows": "int: ctx* int void* size size",
    "upload_founder_panel": "int: ctx* int int u64* size size size",
    "synth_founder_panel": "int: ctx* int int size u64",
    "set_migrant_rows": "int: ctx* int",
    "download_haps": "int: ctx* int int size size u64* size",
    "materialize_pops": "int: ctx* int int size size size size u64** size* size* u64* size",
    "materialize_bed": "int: ctx* int int size size u64** size* size* u8* size",
    "download_snp_major": "int: ctx* int int size size u64* size",
    "format_hap_text": "int: ctx* int int size size u8* size",
    "format_bed": "int: ctx* int int size size u8* size",
    "format_vcf_gt": "int: ctx* int int size size u8* size",
    "snp_genotype_counts": "int: ctx* int int size size size size u32* u32*",
    "dbg_snp_counts_host": "int: u64* size size size size size u32* u32*",
    "ind_genotype_counts": "int: ctx* int int size size size size u32* u32* u32* u64*",
    "pair_genotype_counts": "int: ctx* int int size size size size size size u32* u32* u32*",
    "dbg_pair_counts_host": "int: u64* size size size size size size size size size u32* u32* u32* u32* u32*",
    "ld_counts": "int: ctx* int int size size int size size size size u32* u32* u32* u32* u32* u32* u32* u32*",
    "ld_scores": "int: ctx* int int size size u32* u32* size size int u64* u32*",
    "dbg_ld_host": "int: u64* size size u64* size size size size size size size size size"
                   " u32* u32* u32* u32* u32* u32* u32* u32* u32* u32* int u64* u32*",
    "dbg_ld_r2_q40_host": "int: i64* u64* u64* size u64*",
    "snp_trait_sums": "int: ctx* int int size size size size i32* size i64* i64* u32* u32*",
    "dbg_trait_sums_host": "int: u64* size size size size size size size i32* size i64* i64* u32* u32*",
    "ind_scores": "int: ctx* int int size size size size i32* size i64* i64*",
    "dbg_ind_scores_host": "int: u64* size size size size size size size i32* size i64* i64*",
    "ibd_sharing": "int: ctx* int int size size int size size u64 u64* u32* u64*",
    "ancestry_bp": "int: ctx* int int size size u64* u32*",
    "dbg_ibd_host": "int: part* u64* size part* u64* size u64 u64* u32* u64*",
    "ibd_segments": "int: ctx* int int size size int size size u64 int ibd_segment* size u64*",
    "dbg_ibd_segments_host": "int: part* u64* size part* u64* size u64 int ibd_segment* size u64*",
    "identity_states": "int: ctx* int int size size int size size u64*",
    "dbg_identity_host": "int: part* u64* size part* u64* size u64*",
    "founder_at": "int: ctx* int int size size u64* size u64* u32*",
    "founder_counts": "int: ctx* int int size size u64* size u64* u32* lineage_site* u32*",
    "dbg_lineage_host": "int: part* u64* size u64* size u64* int u32* u32* lineage_site* u32*",
    "dbg_lineage_tile": "u32:",
    "roh_summary": "int: ctx* int int size size size size roh_params* u32* u64* u32* u64* u32*",
    "roh_segments": "int: ctx* int int size size size size roh_params* roh_segment* size u64*",
    "dbg_roh_host": "int: u64* size size size u64* size size size size roh_params* u32* u64* u32* u64* u32* roh_segment* size u64*",
    "rank_f64": "int: ctx* f64* size ull*",
    "download_plink_matrix": "int: ctx* int int size size u64* size",
    "format_ped_text": "int: ctx* int int size size u8* u8* u8* size",
    "set_dense_state": "int: ctx* int",
    "materialize": "int: ctx* int int size size size size u64* size size u64* size",
    "download_cv": "int: ctx* int int int u64* size",
    "download_intervals": "int: ctx* int int part* u64* size*",
    "download_mutations": "int: ctx* int int u64* u64* size*",
    "pop_size": "int: ctx* int size*",
    "plane_ptr": "int: ctx* int int void** size* size* u32** u32*",
    "stitch_totals": "int: ctx* ull* ull* ull* ull*",
    "set_chr_active": "int: ctx* int int",
    "reserve": "int: ctx* int size",
    "stream": "int: ctx* void**",
    "sync": "int: ctx*",
    "set_overlap": "int: ctx* int",
    "last_reproduce_ms": "int: ctx* f32*",
    "timing_totals": "int: ctx* f64* ull*",
    "redo_count": "int: ctx* ull*",
    "compute_ad_device": "int: ctx* int f64** f64** size*",
    "ad_finish_device": "int: ctx* int f64* f64* f64* f64*",
    "list_stats": "int: ctx* int int ull*",
    "set_track_intervals": "int: ctx* int",
    "set_stitch_mode": "int: ctx* int",
    "set_cv_stitch_form": "int: ctx* int",
    "dbg_cv_stitch_launches": "int: ctx* ull*",
    "dbg_verify_planes": "int: ctx* int int u64* ull* ull*",
    "dbg_prefilter_sweep": "int: ctx* u32 u32 ull*",
    "dbg_output_chunk": "int: ctx* size",
    "dbg_bitprod_tiles": "int: ctx* int ull*",
    "dbg_pool_stats": "int: ctx* int ull*",
    "dbg_tables": "int: void* size",
    "dbg_threshold": "int: f64 u32*",
    "dbg_canonical": "f64: u32 u32",
    "dbg_rand": "int: ctx* u32 u32 int*",
    "dbg_sim_loc_rec": "int: ctx* int int u32 u64* u32 u32* int*",
    "dbg_sampling_path": "int: ctx* int*",
    "dbg_ad_path": "int: ctx* int*",
}
ABI_SYMBOLS = list(ABI)

_RETURNS = {"int": C.c_int, "u32": C.c_uint32, "void": None, "f64": C.c_double, "str": C.c_char_p}
_BY_VALUE = {"int": C.c_int, "size": C.c_size_t, "u32": C.c_uint32, "u64": C.c_uint64, "f64": C.c_double, "ctx*": C.c_void_p}
# numpy kinds and item size of a pointer's elements (char* takes bytes and either signedness)
_ELEMENTS = {"int": ("i", C.sizeof(C.c_int)), "i32": ("i", 4), "u32": ("u", 4), "i64": ("i", 8), "u64": ("u", 8),
             "ull": ("u", C.sizeof(C.c_ulonglong)), "size": ("u", C.sizeof(C.c_size_t)), "f32": ("f", 4), "f64": ("f", 8), "u8": ("uiS", 1)}
_void_p = C.c_void_p.from_param


class _Ptr:
    """argtypes entry of a pointer parameter: None, an address, a ctypes instance, array or byref() as c_void_p takes them, or a
    C-contiguous numpy array whose elements fit the parameter (structs by their size, void* anything, pointer-to-pointer none)"""

    def __init__(self, kind):
        self.kind, elem = kind, kind[:-1]
        if elem.endswith("*"):
            self.fits = None
        elif elem == "void":
            self.fits = lambda dt: True
        elif elem in _ELEMENTS:
            kinds, size = _ELEMENTS[elem]
            self.fits = lambda dt: dt.itemsize == size and dt.kind in kinds
        else:
            size = C.sizeof(globals()["gev_" + elem])
            self.fits = lambda dt: dt.itemsize == size

    def from_param(self, a):
        if a is None:
            return None
        if not isinstance(a, np.ndarray):
            return _void_p(a)
        if self.fits is None:
            raise TypeError(f"{self.kind} takes a ctypes array of pointers, not a numpy array")
        if not (a.flags.c_contiguous and self.fits(a.dtype)):
            raise TypeError(f"{self.kind} does not take a{'' if a.flags.c_contiguous else ' non-contiguous'} {a.dtype} array")
        return C.c_void_p(a.ctypes.data)


def _p(a, t=None):
    """address of a numpy array (or None) as a void*, which every pointer parameter takes unchecked.  Nothing in this module needs
    it; raw calls written before the binding was typed wrap their arrays in it and stay valid"""
    return None if a is None else C.c_void_p(a.ctypes.data)


def _arr(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _format_g(f, handle, x):
    x = _arr(x, np.float64).ravel()
    out = np.zeros((len(x), 16), dtype=np.uint8)
    n = C.c_ulonglong()
    args = (x, len(x), out, C.byref(n))
    rc = f(handle, *args) if handle is not None else f(*args)
    return rc, out, int(n.value)


def words_for(nbits):
    return (int(nbits) + 63) // 64


def _rows_out(n_rows, words, stride_words=None):
    """output matrix of `words` words per row; with a wider stride_words it starts as 0xFF bytes, so that what the library wrote shows"""
    if stride_words is None:
        return np.zeros((n_rows, words), dtype=np.uint64)
    assert stride_words >= words
    return np.full((n_rows, stride_words), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


def pack_rows(bits01):
    """uint8 [rows][L] of 0/1 -> uint64 [rows][ceil(L/64)] in the C-ABI packing."""
    b = np.asarray(bits01, dtype=np.uint8)
    pad = (-b.shape[1]) % 64
    if pad:
        b = np.concatenate([b, np.zeros((b.shape[0], pad), dtype=np.uint8)], axis=1)
    return np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little")).view(np.uint64)


def bytes_to_words(packed_u8, L):
    """np.packbits(..., bitorder='little') bytes [rows][ceil(L/8)] -> uint64 words."""
    rows = packed_u8.shape[0]
    w = words_for(L)
    out = np.zeros((rows, w * 8), dtype=np.uint8)
    out[:, :packed_u8.shape[1]] = packed_u8
    return out.view(np.uint64)


def unpack_rows(words, L):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :L]


def _columns(val, n, per):
    """columns as the trait-sum and score calls take them (quanta, weights): int32 [n_cols][n], a single vector as one column.  per: what a
    column holds one value of, for the refusal"""
    val = _arr(val, np.int32)
    if val.ndim == 1:
        val = val.reshape(1, -1)
    assert val.ndim == 2 and val.shape[1] == max(n, 0), f"one {per} of the range"
    return val


def _score_outs(n_scores, n_ind, want=(True, True)):
    """the two matrices of the score calls (None where not wanted)"""
    return tuple(np.empty((n_scores, max(n_ind, 0)), dtype=np.int64) if w else None for w in want)


def _trait_sum_outs(n_traits, n_snps):
    """the two matrices of the trait-sum calls, as the score calls' with SNPs for individuals, and the two count vectors"""
    return (*_score_outs(n_traits, n_snps), np.empty(max(n_snps, 0), dtype=np.uint32), np.empty(max(n_snps, 0), dtype=np.uint32))


def _hap_rows(bits, L, snp_begin, n_snps, ind_begin=0, n_ind=None):
    """what the dbg_*_host calls over haplotype-major rows begin with -> (bits as uint64 [2 * n_people][stride_words], n_people, n_snps,
    n_ind), a range that is None running to the end"""
    bits = _arr(bits, np.uint64)
    assert bits.ndim == 2 and bits.shape[0] % 2 == 0
    n_people = bits.shape[0] // 2
    return bits, n_people, L - snp_begin if n_snps is None else n_snps, n_people - ind_begin if n_ind is None else n_ind


def _ibd_outs(n_a, n_b, want=(True, True, True)):
    """the three matrices of the IBD calls (None where not wanted)"""
    shape = (max(n_a, 0), max(n_b, 0))
    return tuple(np.empty(shape, dtype=dt) if w else None for dt, w in zip((np.uint64, np.uint32, np.uint64), want))


def _founder_haps(n_founder_haps, n_pop):
    """the founder haplotypes per root population as the lineage calls take them: uint64 [n_pop]"""
    nfh = _arr(n_founder_haps, np.uint64)
    assert nfh.shape == (n_pop,), f"one founder count per root population ({n_pop}), {nfh.shape} given"
    return nfh


def _lineage_outs(n_pos, n_rows, n_founders, n_pop, want):
    """(fid, counts, site, pop_counts) of the lineage calls for want = the names wanted (None where not wanted)"""
    n_pos, n_rows = max(n_pos, 0), max(n_rows, 0)
    shapes = {"fid": ((n_pos, n_rows), np.uint32), "counts": ((n_pos, n_founders), np.uint32), "site": ((n_pos,), LINEAGE_SITE_DTYPE),
              "pop_counts": ((n_pos, n_pop), np.uint32)}
    assert set(want) <= set(shapes), want
    return tuple(np.empty(*shapes[k]) if k in want else None for k in ("fid", "counts", "site", "pop_counts"))


def _record_list(call, dtype):
    """the two calls of a record list (IBD segments, runs of homozygosity): call(out, capacity, n_total) counts with (None, 0), then
    fills an exactly sized array of dtype"""
    n = C.c_uint64()
    call(None, 0, C.byref(n))
    out = np.zeros(n.value, dtype=dtype)
    if n.value:
        call(out, n.value, C.byref(n))
        assert n.value == len(out), "the list changed between the count and the fill"
    return out


def _roh_params(min_snps=0, min_bp=0, max_gap_bp=0):
    return gev_roh_params(int(min_snps), 0, int(min_bp), int(max_gap_bp))


def _roh_outs(n_ind, n_snps, want_cover=True):
    """the five vectors of the ROH summary (cover None where not wanted)"""
    n_ind, n_snps = max(n_ind, 0), max(n_snps, 0)
    return (np.empty(n_ind, dtype=np.uint32), np.empty(n_ind, dtype=np.uint64), np.empty(n_ind, dtype=np.uint32), np.empty(n_ind, dtype=np.uint64),
            np.empty(n_snps, dtype=np.uint32) if want_cover else None)


def pack_names(names):
    """list of str / bytes -> (uint8 arena, uint32 offsets [n + 1]) as gev_set_founder_names takes them"""
    b = [x if isinstance(x, bytes) else str(x).encode() for x in names]
    offs = np.zeros(len(b) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(x) for x in b], dtype=np.uint64)
    return np.frombuffer(b"".join(b) + b"\0", dtype=np.uint8).copy(), offs


class GevLibrary:
    def __init__(self, path=DEFAULT_LIB, prefix="gev_", extra_abi=None):
        """extra_abi: lines of ABI's form for functions the library exports beside the header's (the oracle's known-answer helpers)"""
        if not os.path.exists(path):
            raise GevError(-3, f"native library not found: {path} (build it: python -c 'import __graft_entry__ as g; g.build()')")
        self.path, self.prefix = path, prefix
        if prefix == "gev_" and "torch" not in sys.modules:
            # This image holds two HIP runtimes: /opt/rocm's, which the library links, and the one PyTorch-ROCm bundles.  A process
            # that uses both (the bench and the multi-rank tests hand torch's device buffers to the library) must load torch's first:
            # with the library loaded before `import torch`, the runtime initialised second finds no device (measured on the
            # MI355X box: build() followed by smoke() in one process).  Hosts without torch (C++, the bound program) are not affected.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        self.lib = C.CDLL(path)
        self.has_device_arg = prefix == "gev_"
        self.abi = {**ABI, **extra_abi} if extra_abi else ABI
        self._bound = {}

    def _f(self, name):
        """the library's function `name`, typed from the table when it is first looked up"""
        return self._bound.get(name) or self._bind(name)

    def _bind(self, name):
        ret, kinds = self.abi[name].split(":")
        kinds = kinds.split()
        if name == "create" and not self.has_device_arg:
            del kinds[1]
        sym = self.prefix + name
        try:
            cf = getattr(self.lib, sym)
        except AttributeError:
            raise GevError(-5, f"{self.path} does not export {sym}") from None
        cf.restype = _RETURNS[ret]
        cf.argtypes = [_BY_VALUE.get(k) or _Ptr(k) for k in kinds]

        def f(*args):
            if len(args) != len(kinds):         # (ctypes lets surplus arguments through)
                raise TypeError(f"{sym} takes {len(kinds)} arguments ({len(args)} given)")
            try:
                return cf(*args)
            except C.ArgumentError as e:        # "argument <n>: ..." of a by-value conversion or of _Ptr
                raise TypeError(f"{sym}: {e}") from None
        self._bound[name] = f
        return f

    def exports(self, name):
        return hasattr(self.lib, self.prefix + name)

    def last_error(self):
        s = self._f("last_error")()
        return s.decode() if s else ""

    def check(self, rc):
        if rc != 0:
            raise GevError(rc, self.last_error())

    def create(self, n_pop, nchr, nphen, device=-1):
        return GevContext(self, n_pop, nchr, nphen, device)

    def dbg_format_g_host(self, x):
        """printf %g of every double of x by the library's own formatter compiled for the host (no device needed)
        -> (uint8 [n][16], NUL padded; values that took the exact path)"""
        rc, out, n = _format_g(self._f("dbg_format_g_host"), None, x)
        self.check(rc)
        return out, n


    def dbg_snp_counts_host(self, bits, L, snp_begin=0, n_snps=None):
        """(n_het, n_hom_alt) of SNPs [snp_begin, +n_snps) by the library's genotype counter compiled for the host (no device needed).
        bits: uint64 [2 * n_ind][stride_words >= ceil(L / 64)] haplotype-major rows as download_haps returns them"""
        bits, n_people, n_snps, _ = _hap_rows(bits, L, snp_begin, n_snps)
        het = np.empty(n_snps, dtype=np.uint32); hom = np.empty(n_snps, dtype=np.uint32)
        self.check(self._f("dbg_snp_counts_host")(bits, bits.shape[1], n_people, L, snp_begin, n_snps, het, hom))
        return het, hom

    def dbg_pair_counts_host(self, bits, L, snp_begin=0, n_snps=None, a_begin=0, n_a=None, b_begin=0, n_b=None):
        """(n_het, n_hom_alt, n_hethet, n_opphom, dot) by the library's pair counter compiled for the host (no device needed): the first two
        uint32 [n_ind] over SNPs [snp_begin, +n_snps), the others uint32 [n_a][n_b] for the pairs (a_begin + i, b_begin + k).
        bits: uint64 [2 * n_ind][stride_words >= ceil(L / 64)] haplotype-major rows as download_haps returns them"""
        bits, n_ind, n_snps, _ = _hap_rows(bits, L, snp_begin, n_snps)
        n_a = n_ind - a_begin if n_a is None else n_a
        n_b = n_ind - b_begin if n_b is None else n_b
        het = np.empty(n_ind, dtype=np.uint32); hom = np.empty(n_ind, dtype=np.uint32)
        mats = [np.empty((max(n_a, 0), max(n_b, 0)), dtype=np.uint32) for _ in range(3)]
        self.check(self._f("dbg_pair_counts_host")(bits, bits.shape[1], n_ind, L, snp_begin, n_snps, a_begin, n_a, b_begin, n_b, het, hom, *mats))
        return (het, hom, *mats)

    def dbg_ld_host(self, bits_a, L_a, a_begin=0, n_a=None, bits_b=None, L_b=None, b_begin=0, n_b=None, ind_begin=0, n_ind=None,
                    win_lo=None, win_hi=None, genotype=False):
        """the library's LD counter compiled for the host (no device needed).  bits_*: uint64 [2 * n_people][stride_words >= ceil(L / 64)]
        haplotype-major rows as download_haps returns them (bits_b None: side B lies on side A's rows).  Without windows the block form
        -> (n11, gg, c_a, het_a, hom_a, c_b, het_b, hom_b) as GevContext.ld_counts; with win_lo / win_hi (uint32 [n_a]) the score form
        over SNPs [a_begin, +n_a) -> (score_q40 uint64 [n_a], n_terms uint32 [n_a]) as GevContext.ld_scores"""
        bits_a = _arr(bits_a, np.uint64)
        assert bits_a.ndim == 2 and bits_a.shape[0] % 2 == 0
        n_people = bits_a.shape[0] // 2
        n_a = L_a - a_begin if n_a is None else n_a
        n_ind = n_people - ind_begin if n_ind is None else n_ind
        if win_lo is not None or win_hi is not None:
            lo = None if win_lo is None else _arr(win_lo, np.uint32); hi = None if win_hi is None else _arr(win_hi, np.uint32)
            assert all(w is None or w.shape == (n_a,) for w in (lo, hi)), "one window per SNP of the range"
            score = np.empty(max(n_a, 0), dtype=np.uint64); terms = np.empty(max(n_a, 0), dtype=np.uint32)
            self.check(self._f("dbg_ld_host")(bits_a, bits_a.shape[1], L_a, None, 0, 0, n_people, a_begin, n_a, 0, 0, ind_begin, n_ind,
                                              None, None, None, None, None, None, None, None, lo, hi, 1 if genotype else 0, score, terms))
            return score, terms
        if bits_b is None:
            bits_b, L_b = bits_a, L_a
        bits_b = _arr(bits_b, np.uint64)
        assert bits_b.ndim == 2 and bits_b.shape[0] == bits_a.shape[0], "both sides hold the same people"
        n_b = L_b - b_begin if n_b is None else n_b
        mats = [np.empty((max(n_a, 0), max(n_b, 0)), dtype=np.uint32) for _ in range(2)]
        va = [np.empty(max(n_a, 0), dtype=np.uint32) for _ in range(3)]; vb = [np.empty(max(n_b, 0), dtype=np.uint32) for _ in range(3)]
        self.check(self._f("dbg_ld_host")(bits_a, bits_a.shape[1], L_a, bits_b, bits_b.shape[1], L_b, n_people, a_begin, n_a, b_begin, n_b,
                                          ind_begin, n_ind, *mats, *va, *vb, None, None, 0, None, None))
        return (*mats, *va, *vb)

    def dbg_ld_r2_q40_host(self, num, den_j, den_k):
        """the r^2 quantum of every triple (int64 num, uint64 den_j, den_k with num^2 <= den_j * den_k) by the library's function compiled
        for the host -> uint64"""
        num = _arr(num, np.int64).ravel(); den_j = _arr(den_j, np.uint64).ravel(); den_k = _arr(den_k, np.uint64).ravel()
        assert len(num) == len(den_j) == len(den_k)
        out = np.empty(len(num), dtype=np.uint64)
        self.check(self._f("dbg_ld_r2_q40_host")(num, den_j, den_k, len(num), out))
        return out

    def dbg_trait_sums_host(self, bits, L, trait, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None):
        """the library's trait-sum arithmetic compiled for the host (no device needed) -> (gsum, hetsum, n_het, n_hom_alt) as
        GevContext.snp_trait_sums.  bits: uint64 [2 * n_people][stride_words >= ceil(L / 64)] haplotype-major rows as download_haps returns
        them; trait: int32 [n_traits][n_ind] quanta (or [n_ind] for one trait), entry i = individual ind_begin + i"""
        bits, n_people, n_snps, n_ind = _hap_rows(bits, L, snp_begin, n_snps, ind_begin, n_ind)
        trait = _columns(trait, n_ind, "quantum per trait and individual")
        outs = _trait_sum_outs(trait.shape[0], n_snps)
        self.check(self._f("dbg_trait_sums_host")(bits, bits.shape[1], n_people, L, snp_begin, n_snps, ind_begin, n_ind, trait, trait.shape[0], *outs))
        return outs

    def dbg_ind_scores_host(self, bits, L, weight, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None, want=(True, True)):
        """the library's score arithmetic compiled for the host (no device needed) -> (gscore, hetscore) as GevContext.ind_scores.  bits:
        uint64 [2 * n_people][stride_words >= ceil(L / 64)] haplotype-major rows as download_haps returns them; weight: int32
        [n_scores][n_snps] (or [n_snps] for one column), entry j = SNP snp_begin + j"""
        bits, n_people, n_snps, n_ind = _hap_rows(bits, L, snp_begin, n_snps, ind_begin, n_ind)
        weight = _columns(weight, n_snps, "weight per column and SNP")
        outs = _score_outs(weight.shape[0], n_ind, want)
        self.check(self._f("dbg_ind_scores_host")(bits, bits.shape[1], n_people, L, snp_begin, n_snps, ind_begin, n_ind, weight, weight.shape[0], *outs))
        return outs

    def dbg_ibd_host(self, parts_a, off_a, parts_b=None, off_b=None, min_bp=0, want=(True, True, True)):
        """(shared_bp, n_seg, max_seg) of every pair of rows of two sets of interval lists by the library's walk compiled for the host (no
        device needed): uint64 / uint32 / uint64 [n_a][n_b].  parts_* / off_*: as download_intervals returns them (off: rows + 1 entries;
        side b None: side a again); want: an output that is not wanted goes in as NULL and comes back as None"""
        parts_a = _arr(parts_a, PART_DTYPE); off_a = _arr(off_a, np.uint64)
        parts_b = parts_a if parts_b is None else _arr(parts_b, PART_DTYPE); off_b = off_a if off_b is None else _arr(off_b, np.uint64)
        n_a, n_b = len(off_a) - 1, len(off_b) - 1
        outs = _ibd_outs(n_a, n_b, want)
        self.check(self._f("dbg_ibd_host")(parts_a, off_a, n_a, parts_b, off_b, n_b, int(min_bp), *outs))
        return outs

    def dbg_ibd_segments_host(self, parts_a, off_a, parts_b=None, off_b=None, min_bp=0, upper=False):
        """SEGMENT_DTYPE records of every pair of rows of two sets of interval lists by the library's walk compiled for the host (no device
        needed), sorted by (row_a, row_b, st); row_a / row_b index off_a / off_b.  Side b None: side a again, which upper (only pairs
        with row_a < row_b) needs"""
        parts_a = _arr(parts_a, PART_DTYPE); off_a = _arr(off_a, np.uint64)
        parts_b = parts_a if parts_b is None else _arr(parts_b, PART_DTYPE); off_b = off_a if off_b is None else _arr(off_b, np.uint64)
        f, pairs = self._f("dbg_ibd_segments_host"), IBD_UPPER if upper else IBD_ALL_PAIRS
        return _record_list(lambda out, cap, n: self.check(f(parts_a, off_a, len(off_a) - 1, parts_b, off_b, len(off_b) - 1, int(min_bp), pairs, out, cap, n)), SEGMENT_DTYPE)

    def dbg_identity_host(self, parts_a, off_a, parts_b=None, off_b=None):
        """uint64 [9][n_a][n_b]: the base pairs in each of Jacquard's nine identity states of every pair of individuals of two sets of
        interval lists, by the library's four-cursor walk compiled for the host (no device needed).  parts_* / off_*: as
        download_intervals returns them (off: 2 * individuals + 1 entries, rows 2i and 2i+1 are individual i; side b None: side a again)"""
        parts_a = _arr(parts_a, PART_DTYPE); off_a = _arr(off_a, np.uint64)
        parts_b = parts_a if parts_b is None else _arr(parts_b, PART_DTYPE); off_b = off_a if off_b is None else _arr(off_b, np.uint64)
        assert len(off_a) % 2 == 1 and len(off_b) % 2 == 1, "two rows per individual: an odd number of offsets"
        n_a, n_b = (len(off_a) - 1) // 2, (len(off_b) - 1) // 2
        bp = np.empty((9, n_a, n_b), dtype=np.uint64)
        self.check(self._f("dbg_identity_host")(parts_a, off_a, n_a, parts_b, off_b, n_b, bp))
        return bp

    def dbg_lineage_host(self, parts, off, pos, n_founder_haps, want=("fid", "counts", "site", "pop_counts")):
        """(fid, counts, site, pop_counts) as GevContext.founder_at and founder_counts give them, by the library's walk and reductions
        compiled for the host (no device needed).  parts / off: as download_intervals returns them (off: rows + 1 entries); pos: uint64
        positions in non-decreasing order; n_founder_haps: the founder haplotypes of every root population (its length is n_pop); want:
        an output that is not named goes in as NULL and comes back as None"""
        parts = _arr(parts, PART_DTYPE); off = _arr(off, np.uint64); pos = _arr(pos, np.uint64).ravel()
        nfh = _arr(n_founder_haps, np.uint64).ravel()
        n_rows = len(off) - 1
        outs = _lineage_outs(len(pos), n_rows, int(sum(int(x) for x in nfh)) if set(want) & {"counts"} else 0, len(nfh), want)
        self.check(self._f("dbg_lineage_host")(parts, off, n_rows, pos, len(pos), nfh, len(nfh), *outs))
        return outs

    def dbg_lineage_tile(self):
        """founder bins a workgroup of the lineage count kernel histograms at once"""
        return int(self._f("dbg_lineage_tile")())

    def dbg_roh_host(self, bits, L, pos, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None, min_snps=0, min_bp=0, max_gap_bp=0, want_cover=True, want_list=True):
        """the library's run-of-homozygosity word logic compiled for the host (no device needed) -> (n_roh, roh_bp, roh_snps, max_bp, cover,
        segments) as GevContext.roh_summary and roh_segments give them (cover / segments None where not wanted).  bits: uint64
        [2 * n_people][stride_words >= ceil(L / 64)] haplotype-major rows as download_haps returns them; pos: the L SNP positions"""
        bits = _arr(bits, np.uint64); pos = _arr(pos, np.uint64)
        assert bits.ndim == 2 and bits.shape[0] % 2 == 0 and pos.shape == (L,)
        n_people = bits.shape[0] // 2
        n_snps = L - snp_begin if n_snps is None else n_snps
        n_ind = n_people - ind_begin if n_ind is None else n_ind
        q = _roh_params(min_snps, min_bp, max_gap_bp)
        outs = _roh_outs(n_ind, n_snps, want_cover)
        f = self._f("dbg_roh_host")
        head = (bits, bits.shape[1], n_people, L, pos, snp_begin, n_snps, ind_begin, n_ind, C.byref(q))
        if not want_list:
            self.check(f(*head, *outs, None, 0, None))
            return (*outs, None)
        seg = _record_list(lambda out, cap, n: self.check(f(*head, *outs, out, cap, n)), ROH_SEGMENT_DTYPE)
        return (*outs, seg)

    def dbg_format_interval_text_host(self, parts, hap_offsets, ids, chr_label, names, header=True, ind_begin=0, n_ind=None, out_bytes=None):
        """the .int text of individuals [ind_begin, +n_ind) by the library's line formatter compiled for the host (no device needed).
        parts / hap_offsets: as download_intervals returns them; ids: Human::ID of every individual; names: one list of founder
        names per root population.  out_bytes: the buffer's size (None: sized by a size query first) -> bytes"""
        parts = _arr(parts, PART_DTYPE); off = _arr(hap_offsets, np.uint64); ids = _arr(ids, np.int64)
        if n_ind is None:
            n_ind = len(ids) - ind_begin
        packed = [pack_names(x) for x in names]
        npop = len(packed)
        nb_ = (C.c_void_p * max(npop, 1))(*[p[0].ctypes.data for p in packed]); no_ = (C.c_void_p * max(npop, 1))(*[p[1].ctypes.data for p in packed])
        nn = (C.c_size_t * max(npop, 1))(*[len(p[1]) - 1 for p in packed])
        f = self._f("dbg_format_interval_text_host")
        nb = C.c_size_t()
        o, i = off[2 * ind_begin:], ids[ind_begin:]

        def call(buf, size):
            return f(parts, o if len(o) else None, n_ind, i if len(i) else None, chr_label, nb_, no_, nn, npop, 1 if header else 0, buf, size, C.byref(nb))
        if out_bytes is None:
            self.check(call(None, 0))
            out_bytes = nb.value
        buf = np.empty(max(out_bytes, 1), dtype=np.uint8)
        self.last_bytes_written = None
        rc = call(buf, out_bytes)
        self.last_bytes_written = nb.value
        self.check(rc)
        return buf[:nb.value].tobytes()


class GevContext:
    """One simulation context = one GPU (reference: one Simulation object)."""

    def __init__(self, lib, n_pop, nchr, nphen, device=-1):
        self.L, self.n_pop, self.nchr, self.nphen = lib, n_pop, nchr, nphen
        h = C.c_void_p()
        lib.check(lib._f("create")(C.byref(h), *([device] if lib.has_device_arg else []), n_pop, nchr, nphen))
        self.h = h
        self._nsnp = {}
        self._span_bp = {}
        self._snp_span_bp = {}
        self._founder_haps = {}
        self._ncv = {}
        self._chr_off = set()
        self._ph_seeds = 0

    def close(self):
        if self.h:
            self.L._f("destroy")(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        self.L.check(self.L._f(name)(self.h, *args))

    # ---- static inputs
    def set_rmap(self, pop, chr, bp, prob, bp_dist):
        bp = _arr(bp, np.uint64); prob = _arr(prob, np.float64)
        self._call("set_rmap", pop, chr, bp, prob, len(bp), int(bp_dist))
        self._span_bp[(pop, chr)] = int(bp[-1]) - int(bp[0]) if len(bp) else 0     # (the length of a whole-chromosome part: ibd.py)

    def set_mutmap(self, pop, chr, bp, rate):
        bp = _arr(bp, np.uint64); rate = _arr(rate, np.float64)
        self._call("set_mutmap", pop, chr, bp, rate, len(bp))

    def set_snps(self, pop, chr, pos):
        pos = _arr(pos, np.uint64)
        self._nsnp[(pop, chr)] = len(pos)
        self._snp_span_bp[(pop, chr)] = int(pos[-1]) - int(pos[0]) if len(pos) else 0    # (pos[L-1] - pos[0]: the denominator of roh.f_roh)
        self._call("set_snps", pop, chr, pos, len(pos))

    def set_cvs(self, pop, phen, chr, bp, a, d, vd):
        bp = _arr(bp, np.uint64); a = _arr(a, np.float64); d = _arr(d, np.float64)
        self._ncv[(pop, phen, chr)] = len(bp)
        self._call("set_cvs", pop, phen, chr, bp, a, d, len(bp), vd)

    def upload_founders(self, pop, chr, words, L):
        words = _arr(words, np.uint64)
        self._call("upload_founders", pop, chr, words, words.shape[1], words.shape[0], L)
        self._saw_founders(pop, words.shape[0])

    def upload_cv_founders(self, pop, phen, chr, words, ncv):
        words = _arr(words, np.uint64)
        self._call("upload_cv_founders", pop, phen, chr, words, words.shape[1], words.shape[0], ncv)
        self._saw_founders(pop, words.shape[0])

    def synth_founders(self, pop, chr, nhap, seed):
        self._call("synth_founders", pop, chr, nhap, seed)
        self._saw_founders(pop, nhap)

    def upload_founder_panel(self, pop, chr, words, L):
        words = _arr(words, np.uint64)
        self._call("upload_founder_panel", pop, chr, words, words.shape[1], words.shape[0], L)
        self._saw_founders(pop, words.shape[0])

    def synth_founder_panel(self, pop, chr, nhap, seed):
        """read-only founder panel of ROOT population `pop` (immigrants' rows are rebuilt from it, set_migrant_rows(False))"""
        self._call("synth_founder_panel", pop, chr, nhap, seed)
        self._saw_founders(pop, nhap)

    def set_migrant_rows(self, on):
        """False: export_rows packs no genotype rows, import_rows rebuilds them from the founder panels"""
        self._call("set_migrant_rows", 1 if on else 0)

    def synth_cv_founders(self, pop, phen, chr, nhap, seed):
        self._call("synth_cv_founders", pop, phen, chr, nhap, seed)
        self._saw_founders(pop, nhap)

    def _saw_founders(self, pop, nhap):
        """the founder haplotypes of root population `pop`, as its uploads and syntheses gave them (the largest: lineage.py's founder ids)"""
        self._founder_haps[pop] = max(self._founder_haps.get(pop, 0), int(nhap))

    def founder_haps(self, n_founder_haps=None):
        """uint64 [n_pop] as the lineage calls take it: the argument, or what the founder uploads and syntheses of this context said"""
        if n_founder_haps is not None:
            return _founder_haps(n_founder_haps, self.n_pop)
        if len(self._founder_haps) < self.n_pop:
            missing = [p for p in range(self.n_pop) if p not in self._founder_haps]
            raise ValueError(f"n_founder_haps: no founders were uploaded or synthesised for root population(s) {missing}; pass the counts")
        return np.array([self._founder_haps[p] for p in range(self.n_pop)], dtype=np.uint64)

    # ---- generation steps
    def init_gen0(self, pop, n_people, seed_gen0, want_sex=True):
        sex = np.zeros(n_people, dtype=np.uint8) if want_sex else None
        self._call("init_gen0", pop, n_people, int(seed_gen0), sex)
        return sex

    def reproduce(self, pop, couples, seed_reproduce, mut_seeds=None, want_sex=True, n_people=None):
        """couples: int array [n,4] (pos_male,pos_female,inbreed,num_offspring) or COUPLE_DTYPE array;
        None: the couples the preceding random_mate() left in the library (n_people = its pop_size)"""
        if couples is None:
            ms = None if mut_seeds is None else _arr(mut_seeds, np.uint32)
            sex = np.zeros(n_people, dtype=np.uint8) if want_sex else None
            self._call("reproduce", pop, None, 0, int(seed_reproduce), ms, 0 if ms is None else len(ms), n_people, sex)
            return sex
        if couples.dtype != COUPLE_DTYPE:
            c = np.zeros(len(couples), dtype=COUPLE_DTYPE)
            c["pos_male"], c["pos_female"], c["inbreed"], c["num_offspring"] = couples[:, 0], couples[:, 1], couples[:, 2], couples[:, 3]
            couples = c
        couples = np.ascontiguousarray(couples)
        if n_people is None:
            n_people = int(couples["num_offspring"][couples["inbreed"] == 0].sum())
        ms = None if mut_seeds is None else _arr(mut_seeds, np.uint32)
        sex = np.zeros(n_people, dtype=np.uint8) if want_sex else None
        self._call("reproduce", pop, couples, len(couples), int(seed_reproduce), ms, 0 if ms is None else len(ms), n_people, sex)
        return sex

    def reproduce_begin(self, pop, couples, seed_reproduce, mut_seeds=None, n_people=None):
        """first half of reproduce(): stage the inputs and enqueue the generation's device work (returns without waiting)"""
        couples = np.ascontiguousarray(couples)
        assert couples.dtype == COUPLE_DTYPE
        if n_people is None:
            n_people = int(couples["num_offspring"][couples["inbreed"] == 0].sum())
        ms = None if mut_seeds is None else _arr(mut_seeds, np.uint32)
        self._call("reproduce_begin", pop, couples, len(couples), int(seed_reproduce), ms, 0 if ms is None else len(ms), n_people)
        self._pending_people = n_people

    def reproduce_end(self, want_sex=True):
        """second half: wait, redo with larger buffers if needed, publish the generation; returns the sexes"""
        sex = np.zeros(self._pending_people, dtype=np.uint8) if want_sex else None
        self._call("reproduce_end", sex)
        return sex

    def presample_sex(self, pop, n_people):
        """sexes of the generation whose sampling presample() has enqueued (waits for the sampling kernels only)"""
        sex = np.zeros(n_people, dtype=np.uint8)
        self._call("presample_sex", pop, sex, n_people)
        return sex

    def presample(self, pop, seed_reproduce, mut_seeds, n_people):
        """head start for the next reproduce() with the same seeds / n_people (returns without waiting)"""
        ms = None if mut_seeds is None else _arr(mut_seeds, np.uint32)
        self._call("presample", pop, int(seed_reproduce), ms, 0 if ms is None else len(ms), n_people)

    def random_mate(self, pop, seed, selection_value_func, pop_size, want_couples=True):
        """Simulation::random_mate on the library's side -> (couples or None, num_males_mate, num_females_mate)"""
        svf = None if selection_value_func is None else _arr(selection_value_func, np.float64)
        couples = np.zeros(pop_size, dtype=COUPLE_DTYPE) if want_couples else None
        nm, nf = C.c_size_t(), C.c_size_t()
        self._call("random_mate", pop, int(seed), svf, pop_size, couples, C.byref(nm), C.byref(nf))
        return couples, nm.value, nf.value

    def random_mate_selected(self, pop, seed, pop_size, want_couples=True):
        """random_mate() on the selection_value_func compute_selection() left in the library -> (couples or None, num_males_mate, num_females_mate)"""
        couples = np.zeros(pop_size, dtype=COUPLE_DTYPE) if want_couples else None
        nm, nf = C.c_size_t(), C.c_size_t()
        self._call("random_mate_selected", pop, int(seed), pop_size, couples, C.byref(nm), C.byref(nf))
        return couples, nm.value, nf.value

    def _assort_args(self, pop, seeds, pop_size, mat_cor, mm_percent, avoid_inbreeding, offspring_dist, pedigree):
        par = gev_assort_params(int(pop_size), float(mat_cor), float(mm_percent), int(bool(avoid_inbreeding)),
                                ord(offspring_dist) if isinstance(offspring_dist, str) else int(offspring_dist))
        sd = (C.c_uint32 * 4)(*[int(x) for x in (list(seeds) + [0, 0, 0, 0])[:4]])
        ped = None if pedigree is None else _arr(pedigree, np.int64).reshape(-1, 5)
        return par, sd, ped

    def assort_mate(self, pop, seeds, mating_value, selection_value_func, pop_size, mat_cor, mm_percent=0.0, avoid_inbreeding=False,
                    offspring_dist="p", pedigree=None, want_couples=True):
        """Simulation::assort_mate on the library's side -> (couples or None, result dict).  seeds: the 3 (4 with 'p') ras_glob_seed()
        values; selection_value_func None = every value 1; pedigree [n][5] (ID_Father, FF, FM, MF, MM) for avoid_inbreeding.
        The couples stay in the library for reproduce(pop, None, ..., n_people=result["n_offspring"])."""
        par, sd, ped = self._assort_args(pop, seeds, pop_size, mat_cor, mm_percent, avoid_inbreeding, offspring_dist, pedigree)
        mv = _arr(mating_value, np.float64)
        svf = None if selection_value_func is None else _arr(selection_value_func, np.float64)
        couples = np.zeros(len(mv), dtype=COUPLE_DTYPE) if want_couples else None      # n_couples <= n_people
        res = gev_assort_result()
        self._call("assort_mate", pop, C.byref(par), sd, mv, svf, ped, couples, C.byref(res))
        r = _assort_result(res)
        return (couples[:r["n_couples"]].copy() if want_couples else None), r

    def assort_mate_selected(self, pop, seeds, pop_size, mat_cor, mm_percent=0.0, avoid_inbreeding=False, offspring_dist="p",
                             pedigree=None, want_couples=True):
        """assort_mate() on the mating values and selection_value_func compute_selection() left in the library"""
        par, sd, ped = self._assort_args(pop, seeds, pop_size, mat_cor, mm_percent, avoid_inbreeding, offspring_dist, pedigree)
        couples = np.zeros(self.pop_size(pop), dtype=COUPLE_DTYPE) if want_couples else None
        res = gev_assort_result()
        self._call("assort_mate_selected", pop, C.byref(par), sd, ped, couples, C.byref(res))
        r = _assort_result(res)
        return (couples[:r["n_couples"]].copy() if want_couples else None), r

    def last_assort_result(self, want_couples=False):
        """-> (result dict, couples or None) of the context's last completed assort_mate()"""
        res = gev_assort_result()
        self._call("last_assort_result", C.byref(res), None)
        r = _assort_result(res)
        couples = None
        if want_couples:
            couples = np.zeros(r["n_couples"], dtype=COUPLE_DTYPE)
            self._call("last_assort_result", C.byref(res), couples)
        return r, couples

    def dbg_assort_knobs(self, narrow_window=False, short_poisson=False):
        """set the test hooks of the exact fallbacks for the following assort_mate() calls (both off by default)"""
        self._call("dbg_assort_knobs", int(bool(narrow_window)), int(bool(short_poisson)))

    def dbg_assort_stats(self):
        """-> {chunks, direct, pois_reruns} of the last assort_mate()"""
        out = (C.c_ulonglong * 3)()
        self._call("dbg_assort_stats", out)
        return {"chunks": int(out[0]), "direct": int(out[1]), "pois_reruns": int(out[2])}

    def generation_begin_assort(self, pop, glob_state, pop_size, mat_cor, mm_percent=0.0, avoid_inbreeding=False, offspring_dist="p",
                                mating_value=None, selection_value_func=None, pedigree=None, selected=False):
        """assort_mate -> reproduce -> ras_compute_AD of one generation as one call pair, every seed drawn by the library from glob_state
        (returns once the mating counts are known, without waiting for the rest); selected=True: on the values compute_selection()
        left in the library.  -> the assort result dict (n_couples, n_offspring, ...) of this generation"""
        par, _, ped = self._assort_args(pop, (), pop_size, mat_cor, mm_percent, avoid_inbreeding, offspring_dist, pedigree)
        if selected:
            self._call("generation_begin_assort_selected", pop, int(glob_state), C.byref(par), ped)
        else:
            mv = _arr(mating_value, np.float64)
            svf = None if selection_value_func is None else _arr(selection_value_func, np.float64)
            self._call("generation_begin_assort", pop, int(glob_state), C.byref(par), mv, svf, ped)
        r, _ = self.last_assort_result()
        self._pending_people, self._pending_couples = r["n_offspring"], r["n_couples"]
        return r

    def set_track_pedigree(self, on):
        """True (before init_gen0): the library keeps the seven pedigree ids of every individual on the device"""
        self._call("set_track_pedigree", 1 if on else 0)

    def download_pedigree(self, pop):
        """-> int64 [n_people][7]: ID, ID_Father, ID_Mother, ID_Fathers_Father, ID_Fathers_Mother, ID_Mothers_Father, ID_Mothers_Mother"""
        ids = np.zeros((self.pop_size(pop), 7), dtype=np.int64)
        self._call("download_pedigree", pop, ids)
        return ids

    def upload_pedigree(self, pop, ids):
        """restore the ids of the population's current individuals ([n_people][7] as download_pedigree) after remove_rows / import_rows"""
        ids = _arr(ids, np.int64)
        if ids.shape != (self.pop_size(pop), 7):
            raise ValueError("upload_pedigree: one row of 7 ids per individual expected")
        self._call("upload_pedigree", pop, ids)

    def generation_phenotypes(self, pop, gen_num, glob_state, schemes, vt_type=1):
        """ras_scale_AD_compute_GEF for every phenotype from the library's own state (enqueues only).  schemes: one (va, vd, vc, ve,
        vf, beta) per phenotype"""
        if len(schemes) != self.nphen:
            raise ValueError("generation_phenotypes: one scheme per phenotype expected")
        sch = (gev_pheno_scheme * self.nphen)(*[gev_pheno_scheme(*[float(x) for x in s]) for s in schemes])
        par = gev_phenotypes_params(int(gen_num), int(vt_type), C.cast(sch, C.c_void_p))
        self._call("generation_phenotypes", pop, C.byref(par), int(glob_state))
        self._ph_seeds = (self.nphen + sum(1 for s in schemes if s[2] > 0)) if gen_num == 0 else self.nphen

    def phenotypes_result(self, pop):
        """waits -> dict(glob_state, seeds (uint32, draw order), var [nphen][7] of A D G C E F P)"""
        st = C.c_uint32(); seeds = np.zeros(2 * self.nphen, dtype=np.uint32); var = np.zeros((self.nphen, 7))      # (at most two seeds per phenotype)
        self._call("phenotypes_result", pop, C.byref(st), seeds, var)
        return {"glob_state": st.value, "seeds": seeds[:self._ph_seeds].copy(), "var": var}

    def download_phenotypes(self, pop, phen):
        """-> dict of the seven n-vectors of PHENOTYPE_COMPONENTS"""
        out = np.zeros((7, self.pop_size(pop)))
        self._call("download_phenotypes", pop, phen, out)
        return dict(zip(PHENOTYPE_COMPONENTS, out))

    def get_ad_gen0(self, pop, phen):
        a, d = C.c_double(), C.c_double()
        self._call("get_ad_gen0", pop, phen, C.byref(a), C.byref(d))
        return a.value, d.value

    def set_ad_gen0(self, pop, phen, var_a, var_d):
        self._call("set_ad_gen0", pop, phen, var_a, var_d)

    def save_prev_gen(self, pop, phen_shift=None):
        sh = None if phen_shift is None else _arr(phen_shift, np.float64)
        if sh is not None and len(sh) != self.nphen:
            raise ValueError("save_prev_gen: one shift per phenotype expected")
        self._call("save_prev_gen", pop, sh)

    def upload_prev_gen(self, pop, phen, parental_effect):
        """the saved record from the host: [nphen][n] each (None = zeros)"""
        ph = None if phen is None else _arr(phen, np.float64).reshape(self.nphen, -1)
        pe = None if parental_effect is None else _arr(parental_effect, np.float64).reshape(self.nphen, -1)
        n = (ph if ph is not None else pe).shape[1]
        if ph is not None and pe is not None and ph.shape != pe.shape:
            raise ValueError("upload_prev_gen: phen and parental_effect differ in shape")
        self._call("upload_prev_gen", pop, ph, pe, n)

    def info_row_bytes(self):
        """the largest possible row of format_info_text"""
        return 7 * 21 + 2 + (7 * self.nphen + 3) * 14

    def format_info_text(self, pop, ind_begin=0, n_ind=None, header=True):
        """bytes of the reference's .info file (Population::ras_save_human_info) for individuals [ind_begin, ind_begin + n_ind) of the
        current generation, formatted on the device; header: with the header line in front"""
        if n_ind is None:
            n_ind = self.pop_size(pop) - ind_begin
        cap = 128 + 56 * self.nphen + max(int(n_ind), 0) * self.info_row_bytes()
        buf = getattr(self, "_info_buf", None)
        if buf is None or len(buf) < cap:                   # kept: a fresh buffer of this size costs more page faults than the copy-out
            buf = self._info_buf = np.empty(cap, dtype=np.uint8)
        nb = C.c_size_t()
        self._call("format_info_text", pop, ind_begin, n_ind, 1 if header else 0, buf, len(buf), C.byref(nb))
        return buf[:nb.value].tobytes()

    def info_text_size(self, pop, ind_begin=0, n_ind=None, header=True):
        """the exact size format_info_text() would return (length pass only)"""
        if n_ind is None:
            n_ind = self.pop_size(pop) - ind_begin
        nb = C.c_size_t()
        self._call("format_info_text", pop, ind_begin, n_ind, 1 if header else 0, None, 0, C.byref(nb))
        return nb.value

    def set_founder_names(self, root_pop, names):
        """the founder individuals' names (the .indv file) of a root population, for format_interval_text"""
        arena, offs = pack_names(names)
        self._call("set_founder_names", root_pop, arena, offs, len(offs) - 1)

    def format_interval_text(self, pop, chr, chr_label, ind_begin=0, n_ind=None, header=True, ids=None):
        """bytes of the reference's .int file (Simulation::ras_write_hap_to_interval_format) for individuals [ind_begin, ind_begin +
        n_ind) of (pop, chr), formatted on the device.  ids: Human::ID of those n_ind individuals, None = the ids the library tracks"""
        if n_ind is None:
            n_ind = self.pop_size(pop) - ind_begin
        if ids is not None:
            ids = _arr(ids, np.int64)
            if len(ids) != n_ind:
                raise ValueError("format_interval_text: one id per individual of the range expected")
        size = self.interval_text_size(pop, chr, chr_label, ind_begin, n_ind, header, ids)
        buf = np.empty(max(size, 1), dtype=np.uint8)
        nb = C.c_size_t()
        self._call("format_interval_text", pop, chr, chr_label, ind_begin, n_ind, 1 if header else 0, ids, buf, size, C.byref(nb))
        return buf[:nb.value].tobytes()

    def interval_text_size(self, pop, chr, chr_label, ind_begin=0, n_ind=None, header=True, ids=None):
        """the exact size format_interval_text() would return (length pass only)"""
        if n_ind is None:
            n_ind = self.pop_size(pop) - ind_begin
        ids = None if ids is None else _arr(ids, np.int64)
        nb = C.c_size_t()
        self._call("format_interval_text", pop, chr, chr_label, ind_begin, n_ind, 1 if header else 0, ids, None, 0, C.byref(nb))
        return nb.value

    def dbg_format_g(self, x):
        """printf %g of every double of x on the device -> (uint8 [n][16], NUL padded; values that took the exact path)"""
        rc, out, n = _format_g(self.L._f("dbg_format_g"), self.h, x)
        self.L.check(rc)
        return out, n

    def dbg_phenotype_knobs(self, short_candidates=False):
        """-> phenotype steps and scale_ad_compute_gef() calls run again so far; short_candidates: start their normal streams far too short"""
        n = C.c_ulonglong()
        self._call("dbg_phenotype_knobs", int(bool(short_candidates)), C.byref(n))
        return int(n.value)

    def compute_selection(self, pop, gen_num, func, par1, par2, omega, lambda_, phen_shift=None, want=("mating_value", "selection_value", "selection_value_func")):
        """Simulation::ras_compute_mating_value_selection_value + ras_selection_func on the device, from the phenotypes the last
        scale_ad_compute_gef() of every phenotype left there.  func: a key of SELECTION_FUNCS (the reference's name; None = "none")
        or a GEV_SEL_* code.  -> dict of the n-vectors named in `want` (empty `want`: enqueued only, nothing waits)."""
        code = SELECTION_FUNCS[func if func is not None else "none"] if not isinstance(func, int) else func
        om, la = _arr(omega, np.float64), _arr(lambda_, np.float64)
        sh = None if phen_shift is None else _arr(phen_shift, np.float64)
        if len(om) != self.nphen or len(la) != self.nphen or (sh is not None and len(sh) != self.nphen):
            raise ValueError("omega / lambda_ / phen_shift need one value per phenotype")
        par = gev_selection_params(int(gen_num), code, float(par1), float(par2), om.ctypes.data, la.ctypes.data, None if sh is None else sh.ctypes.data)
        n = self.pop_size(pop) if want else 0
        out = {k: np.zeros(n) for k in want}
        self._call("compute_selection", pop, C.byref(par), out.get("mating_value"), out.get("selection_value"), out.get("selection_value_func"))
        return out

    def download_selection(self, pop):
        """-> dict(mating_value, selection_value, selection_value_func) the library holds for the population's current generation"""
        n = self.pop_size(pop)
        out = {k: np.zeros(n) for k in ("mating_value", "selection_value", "selection_value_func")}
        self._call("download_selection", pop, out["mating_value"], out["selection_value"], out["selection_value_func"])
        return out

    def get_selection_gen0(self, pop):
        """-> (_gen0_SV_mean, _gen0_SV_var) of the population"""
        m, v = C.c_double(), C.c_double()
        self._call("get_selection_gen0", pop, C.byref(m), C.byref(v))
        return m.value, v.value

    def set_selection_gen0(self, pop, mean, var):
        self._call("set_selection_gen0", pop, mean, var)

    def glob_seeds(self, engine_state, n, want=True):
        """n Simulation::ras_glob_seed() values from glob_generator's state -> (values or None, state after)"""
        st = C.c_uint32(int(engine_state))
        out = np.zeros(n, dtype=np.uint32) if want else None
        self._call("glob_seeds", C.byref(st), n, out)
        return out, st.value

    def generation_begin(self, pop, glob_state, pop_size, selection_value_func=None):
        """random_mate -> reproduce -> ras_compute_AD of one generation, enqueued as one unit (returns without waiting)"""
        svf = None if selection_value_func is None else _arr(selection_value_func, np.float64)
        self._call("generation_begin", pop, int(glob_state), pop_size, svf)
        self._pending_people = self._pending_couples = pop_size

    def generation_begin_selected(self, pop, glob_state, pop_size):
        """generation_begin() mating on the selection_value_func compute_selection() left in the library (nothing uploaded)"""
        self._call("generation_begin_selected", pop, int(glob_state), pop_size)
        self._pending_people = self._pending_couples = pop_size

    def generation_end(self, want_couples=False, want_sex=True):
        """-> dict(glob_state, seed_mate, seed_reproduce, num_males_mate, num_females_mate, couples, sex)"""
        res = gev_generation_result()
        couples = np.zeros(self._pending_couples, dtype=COUPLE_DTYPE) if want_couples else None
        sex = np.zeros(self._pending_people, dtype=np.uint8) if want_sex else None
        self._call("generation_end", C.byref(res), couples, sex)
        return {"glob_state": res.glob_state, "seed_mate": res.seed_mate, "seed_reproduce": res.seed_reproduce,
                "num_males_mate": res.num_males_mate, "num_females_mate": res.num_females_mate, "couples": couples, "sex": sex}

    def set_generation_chain(self, draws_between):
        """ras_glob_seed() draws the host makes itself between two generation_begin() calls (None: unknown, no head start)"""
        self._call("set_generation_chain", -1 if draws_between is None else int(draws_between))

    def compute_ad_device(self, pop):
        """gev_compute_ad_device: (device pointer of the per-chromosome additive array, ... of the dominance array, length in doubles)"""
        a, d, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._call("compute_ad_device", pop, C.byref(a), C.byref(d), C.byref(n))
        return int(a.value), int(d.value), int(n.value)

    def ad_finish_device(self, pop, per_chr=True):
        """gev_ad_finish_device -> (additive, dominance, additive_chr, dominance_chr) after the caller's in-place all-reduce"""
        n = self.pop_size(pop)
        add = np.zeros((n, self.nphen)); dom = np.zeros((n, self.nphen))
        addc = np.zeros((n, self.nchr, self.nphen)) if per_chr else None; domc = np.zeros((n, self.nchr, self.nphen)) if per_chr else None
        self._call("ad_finish_device", pop, add, dom, addc, domc)
        return add, dom, addc, domc

    def list_stats(self, pop=0, chrom=0):
        """gev_list_stats as a dict"""
        out = (C.c_ulonglong * 10)()
        self._call("list_stats", pop, chrom, out)
        keys = ("rebuilds", "interval_entries_used", "mutation_entries_used", "interval_capacity", "mutation_capacity", "ranges_per_row", "interval_entries_last_generation", "mutation_entries_last_generation", "compactions", "reserved")
        return dict(zip(keys, (int(v) for v in out)))

    def redo_count(self):
        n = C.c_ulonglong()
        self._call("redo_count", C.byref(n))
        return n.value

    def dbg_pool_stats(self, pop):
        """-> (rebuilds of the free list of the population's segment unit pool, generations enqueued again because it ran out)"""
        out = (C.c_ulonglong * 2)()
        self._call("dbg_pool_stats", pop, out)
        return int(out[0]), int(out[1])

    def compute_ad(self, pop, per_chr=True):
        n = self.pop_size(pop)
        add = np.zeros((n, self.nphen)); dom = np.zeros((n, self.nphen))
        addc = np.zeros((n, self.nchr, self.nphen)) if per_chr else None
        domc = np.zeros((n, self.nchr, self.nphen)) if per_chr else None
        self._call("compute_ad", pop, add, dom, addc, domc)
        return add, dom, addc, domc

    def scale_ad_compute_gef(self, pop, phen, gen_num, seed, va, vd, ve, vf, beta, s2_a_gen0, s2_d_gen0,
                             common_sibling=None, f_father=None, f_mother=None):
        """Simulation::ras_scale_AD_compute_GEF (reference src/Simulation.cpp:3075): -> dict of n-vectors"""
        n = self.pop_size(pop)
        par = gev_gef_params(va, vd, ve, vf, beta, s2_a_gen0, s2_d_gen0, gen_num, 0)
        arr = lambda x: None if x is None else _arr(x, np.float64)
        cs, ff, fm = arr(common_sibling), arr(f_father), arr(f_mother)
        out = {k: np.zeros(n) for k in ("additive", "dominance", "bv", "e_noise", "parental_effect", "phen")}
        self._call("scale_ad_compute_gef", pop, phen, C.byref(par), int(seed), cs, ff, fm,
                   out["additive"], out["dominance"], out["bv"], out["e_noise"], out["parental_effect"], out["phen"])
        return out

    def set_ad(self, pop, additive, dominance):
        """raw A/D totals of the current generation from the host (locus-split populations: the all-reduced sums)"""
        a = _arr(additive, np.float64); d = _arr(dominance, np.float64)
        self._call("set_ad", pop, a, d)

    def get_cv_freq(self, pop, phen, chr):
        ncv = self._ncv[(pop, phen, chr)]
        f = np.zeros(ncv)
        self._call("get_cv_freq", pop, phen, chr, f, ncv)
        return f

    def migrate(self, moves):
        """moves: list/array of (src_pop, src_pos, dst_pop) in reference append order"""
        m = np.zeros(len(moves), dtype=MOVE_DTYPE)
        for i, (sp, pos, dp) in enumerate(moves):
            m[i] = (sp, dp, pos)
        self._call("migrate", m, len(m))

    # ---- downloads
    def pop_size(self, pop):
        n = C.c_size_t()
        self._call("pop_size", pop, C.byref(n))
        return n.value

    # a count given as None: the rest of the SNPs of (pop, chr) / of the individuals (per_individual 2: haplotype rows) of pop from `begin` on
    def _rest_snps(self, pop, chr, begin, n):
        return self._nsnp[(pop, chr)] - begin if n is None else n

    def _rest_ind(self, pop, begin, n, per_individual=1):
        return per_individual * self.pop_size(pop) - begin if n is None else n

    def dbg_output_chunk(self, max_units=0):
        """test hook: the following output calls stage at most max_units rows / individuals / SNPs (SNPs in 64s) per pass; 0 = byte budgets"""
        self._call("dbg_output_chunk", max_units)

    def dbg_bitprod_tiles(self, mode=-1):
        """test hook: the tile size of the following pair-count / LD products (0 = by compute units, 1 = always 64 x 64, 2 = always
        128 x 128, -1 = unchanged) -> (small, large): the product launches on either size since the context was created"""
        n = (C.c_ulonglong * 2)()
        self._call("dbg_bitprod_tiles", mode, n)
        return int(n[0]), int(n[1])

    def download_haps(self, pop, chr, row_begin=0, n_rows=None, stride_words=None):
        L = self._nsnp[(pop, chr)]
        if n_rows is None:
            n_rows = 2 * self.pop_size(pop) - row_begin
        out = _rows_out(n_rows, words_for(L), stride_words)
        self._call("download_haps", pop, chr, row_begin, n_rows, out, out.shape[1])
        return out

    def download_snp_major(self, pop, chr, snp_begin=0, n_snps=None, stride_words=None):
        L = self._nsnp[(pop, chr)]
        n_snps = L - snp_begin if n_snps is None else n_snps
        out = _rows_out(n_snps, words_for(2 * self.pop_size(pop)), stride_words)
        self._call("download_snp_major", pop, chr, snp_begin, n_snps, out, out.shape[1])
        return out

    def snp_genotype_counts(self, pop, chr, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None):
        """-> (n_het, n_hom_alt), uint32 [n_snps]: per SNP of the range, the individuals of [ind_begin, +n_ind) that are heterozygous /
        carry allele 1 twice, counted on the device from the resident rows (mutations applied)"""
        n_snps = self._rest_snps(pop, chr, snp_begin, n_snps)
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        het = np.empty(max(n_snps, 0), dtype=np.uint32); hom = np.empty(max(n_snps, 0), dtype=np.uint32)
        self._call("snp_genotype_counts", pop, chr, snp_begin, n_snps, ind_begin, n_ind, het, hom)
        return het, hom

    def allele_freq(self, pop, chr, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None):
        """-> float64 [n_snps]: frequency of allele 1 among the 2 * n_ind haplotypes of the individuals of the range"""
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        het, hom = self.snp_genotype_counts(pop, chr, snp_begin, n_snps, ind_begin, n_ind)
        return (het.astype(np.float64) + 2.0 * hom) / (2.0 * n_ind)

    def ind_genotype_counts(self, pop, chr, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None, weight=None):
        """-> (n_het, n_hom_alt) uint32 [n_ind], or with weight (n_snps uint32) (n_het, n_hom_alt, wsum), wsum uint64 [n_ind] =
        sum_j weight[j] * g_ij: per individual of the range over the SNPs of the range, counted on the device (mutations applied)"""
        n_snps = self._rest_snps(pop, chr, snp_begin, n_snps)
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        het = np.empty(max(n_ind, 0), dtype=np.uint32); hom = np.empty(max(n_ind, 0), dtype=np.uint32)
        ws = None
        if weight is not None:
            weight = _arr(weight, np.uint32)
            assert weight.shape == (n_snps,), "one weight per SNP of the range"
            ws = np.empty(max(n_ind, 0), dtype=np.uint64)
        self._call("ind_genotype_counts", pop, chr, snp_begin, n_snps, ind_begin, n_ind, weight, het, hom, ws)
        return (het, hom) if weight is None else (het, hom, ws)

    def pair_genotype_counts(self, pop, chr, snp_begin=0, n_snps=None, a_begin=0, n_a=None, b_begin=0, n_b=None):
        """-> (n_hethet, n_opphom, dot), uint32 [n_a][n_b]: for every pair (a_begin + i, b_begin + k) of the population over the SNPs of the
        range, the loci where both are heterozygous, the loci where one is 0/0 and the other 1/1, and sum_j g_ij g_kj; exact integer
        products on the device's matrix cores from the resident rows (mutations applied)"""
        n_snps = self._rest_snps(pop, chr, snp_begin, n_snps)
        n_a = self._rest_ind(pop, a_begin, n_a)
        n_b = self._rest_ind(pop, b_begin, n_b)
        mats = [np.empty((max(n_a, 0), max(n_b, 0)), dtype=np.uint32) for _ in range(3)]
        self._call("pair_genotype_counts", pop, chr, snp_begin, n_snps, a_begin, n_a, b_begin, n_b, *mats)
        return tuple(mats)

    def ld_counts(self, pop, chr_a, a_begin=0, n_a=None, chr_b=None, b_begin=0, n_b=None, ind_begin=0, n_ind=None):
        """-> (n11, gg, c_a, het_a, hom_a, c_b, het_b, hom_b): for SNP j of [a_begin, +n_a) of chr_a and SNP k of [b_begin, +n_b) of chr_b
        (None: chr_a) over individuals [ind_begin, +n_ind), uint32 [n_a][n_b]: n11 = haplotypes with allele 1 at both, gg = sum_i g_ij g_ik;
        per SNP of each side, uint32: allele-1 count, heterozygous and homozygous-alt individuals.  Exact integer products on the device's
        matrix cores from the current generation (mutations applied)"""
        chr_b = chr_a if chr_b is None else chr_b
        n_a = self._rest_snps(pop, chr_a, a_begin, n_a)
        n_b = self._rest_snps(pop, chr_b, b_begin, n_b)
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        mats = [np.empty((max(n_a, 0), max(n_b, 0)), dtype=np.uint32) for _ in range(2)]
        vecs = [np.empty(max(n, 0), dtype=np.uint32) for n in (n_a, n_a, n_a, n_b, n_b, n_b)]
        self._call("ld_counts", pop, chr_a, a_begin, n_a, chr_b, b_begin, n_b, ind_begin, n_ind, *mats, *vecs)
        return (*mats, *vecs)

    def ld_scores(self, pop, chr, win_lo, win_hi, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None, genotype=False):
        """-> (score_q40 uint64 [n_snps], n_terms uint32 [n_snps]): for SNP snp_begin + t the sum over SNPs [win_lo[t], win_hi[t]) of the
        chromosome of the r^2 quantum llrint(r^2 * 2^40) (haplotype r^2, or genotype r^2) over individuals [ind_begin, +n_ind), and the
        window's SNPs that are polymorphic among them; the band is walked and reduced on the device"""
        n_snps = self._rest_snps(pop, chr, snp_begin, n_snps)
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        lo = _arr(win_lo, np.uint32); hi = _arr(win_hi, np.uint32)
        assert lo.shape == hi.shape == (max(n_snps, 0),), "one window per SNP of the range"
        score = np.empty(max(n_snps, 0), dtype=np.uint64); terms = np.empty(max(n_snps, 0), dtype=np.uint32)
        self._call("ld_scores", pop, chr, snp_begin, n_snps, lo, hi, ind_begin, n_ind, 1 if genotype else 0, score, terms)
        return score, terms

    def snp_trait_sums(self, pop, chr, trait, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None):
        """-> (gsum, hetsum, n_het, n_hom_alt): for SNP j of [snp_begin, +n_snps) and trait t over individuals [ind_begin, +n_ind), int64
        [n_traits][n_snps]: gsum = sum_i g_ij q[t][i], hetsum = the sum of q[t][i] over the heterozygous individuals; uint32 [n_snps]: the
        heterozygous and homozygous-alt individuals.  trait: int32 [n_traits][n_ind] quanta, |q| <= 2^30 (or [n_ind] for one trait), entry
        i = individual ind_begin + i.  Exact integer products on the device's matrix cores from the current generation (mutations applied)"""
        n_snps = self._rest_snps(pop, chr, snp_begin, n_snps)
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        trait = _columns(trait, n_ind, "quantum per trait and individual")
        outs = _trait_sum_outs(trait.shape[0], n_snps)
        self._call("snp_trait_sums", pop, chr, snp_begin, n_snps, ind_begin, n_ind, trait, trait.shape[0], *outs)
        return outs

    def ind_scores(self, pop, chr, weight, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None, want=(True, True)):
        """-> (gscore, hetscore), int64 [n_scores][n_ind]: for individual i of [ind_begin, +n_ind) and column s over SNPs [snp_begin,
        +n_snps), gscore = sum_j w[s][j] g_ij, hetscore = the sum of w[s][j] over the SNPs at which i is heterozygous.  weight: int32
        [n_scores][n_snps], |w| <= 2^30 (or [n_snps] for one column), entry j = SNP snp_begin + j; at most 2^22 SNPs a call (the sums
        are additive: scores.sums splits).  Exact integer products on the device's matrix cores from the current generation (mutations
        applied).  want: an output that is not wanted goes in as NULL and comes back as None"""
        n_snps = self._rest_snps(pop, chr, snp_begin, n_snps)
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        weight = _columns(weight, n_snps, "weight per column and SNP")
        outs = _score_outs(weight.shape[0], n_ind, want)
        self._call("ind_scores", pop, chr, snp_begin, n_snps, ind_begin, n_ind, weight, weight.shape[0], *outs)
        return outs

    def ibd_sharing(self, chr, pop_a, a_begin=0, n_a=None, pop_b=None, b_begin=0, n_b=None, min_bp=0, want=(True, True, True)):
        """-> (shared_bp, n_seg, max_seg), uint64 / uint32 / uint64 [n_a][n_b]: for haplotype row a_begin + i of pop_a against row b_begin + k
        of pop_b (None: pop_a), over the segments of at least min_bp base pairs along which both descend from the same founder haplotype:
        their summed length, their number and the longest.  Walked on the device from the ancestry interval lists (works without genotype
        planes).  want: an output that is not wanted goes in as NULL and comes back as None"""
        pop_b = pop_a if pop_b is None else pop_b
        n_a = self._rest_ind(pop_a, a_begin, n_a, 2)
        n_b = self._rest_ind(pop_b, b_begin, n_b, 2)
        outs = _ibd_outs(n_a, n_b, want)
        self._call("ibd_sharing", chr, pop_a, a_begin, n_a, pop_b, b_begin, n_b, int(min_bp), *outs)
        return outs

    def ibd_segments(self, chr, pop_a, a_begin=0, n_a=None, pop_b=None, b_begin=0, n_b=None, min_bp=0, upper=False):
        """-> SEGMENT_DTYPE records (st, en, row_a, row_b), sorted by (row_a, row_b, st): the segments of at least min_bp base pairs along
        which row a_begin + i of pop_a and row b_begin + k of pop_b (None: pop_a) descend from the same founder haplotype, [st, en), the
        rows absolute in their populations.  upper: only pairs with row_a < row_b (one population).  A count call, then a fill call"""
        pop_b = pop_a if pop_b is None else pop_b
        n_a = self._rest_ind(pop_a, a_begin, n_a, 2)
        n_b = self._rest_ind(pop_b, b_begin, n_b, 2)
        pairs = IBD_UPPER if upper else IBD_ALL_PAIRS
        return _record_list(lambda out, cap, n: self._call("ibd_segments", chr, pop_a, a_begin, n_a, pop_b, b_begin, n_b, int(min_bp), pairs, out, cap, n), SEGMENT_DTYPE)

    def identity_states(self, chr, pop_a, a_begin=0, n_a=None, pop_b=None, b_begin=0, n_b=None):
        """-> uint64 [9][n_a][n_b]: for individual a_begin + i of pop_a against individual b_begin + k of pop_b (None: pop_a), plane s - 1 =
        the base pairs of the chromosome at which the four haplotypes are in Jacquard's condensed identity state s (all four covered):
        1 all four IBD, 2 each autozygous, 3 / 4 a autozygous with / without sharing, 5 / 6 b likewise, 7 both pairs across, 8 one
        pair across, 9 nothing shared.  Walked on the device from the ancestry interval lists (works without genotype planes);
        identity.py has the statistics"""
        pop_b = pop_a if pop_b is None else pop_b
        n_a = self._rest_ind(pop_a, a_begin, n_a)
        n_b = self._rest_ind(pop_b, b_begin, n_b)
        bp = np.empty((9, max(n_a, 0), max(n_b, 0)), dtype=np.uint64)
        self._call("identity_states", chr, pop_a, a_begin, n_a, pop_b, b_begin, n_b, bp)
        return bp

    def founder_at(self, pop, chr, pos, row_begin=0, n_rows=None, n_founder_haps=None):
        """-> fid uint32 [n_pos][n_rows]: the founder id of haplotype row row_begin + i at pos[p] (uint64, non-decreasing): base[root
        population] + hap_index of the part that covers the position, base the exclusive prefix sum of n_founder_haps (None: what the
        founder uploads and syntheses said); NO_FOUNDER where no part covers it.  Walked on the device from the ancestry interval lists"""
        n_rows = self._rest_ind(pop, row_begin, n_rows, 2)
        pos = _arr(pos, np.uint64).ravel(); nfh = self.founder_haps(n_founder_haps)
        fid = _lineage_outs(len(pos), n_rows, 0, self.n_pop, ("fid",))[0]
        self._call("founder_at", pop, chr, row_begin, n_rows, pos, len(pos), nfh, fid)
        return fid

    def founder_counts(self, pop, chr, pos, row_begin=0, n_rows=None, n_founder_haps=None, want=("counts", "site", "pop_counts")):
        """-> (counts uint32 [n_pos][F], site LINEAGE_SITE_DTYPE [n_pos], pop_counts uint32 [n_pos][n_pop]) per position over the haplotype
        rows [row_begin, +n_rows): the rows by founder id, their summary (sum_sq, n_covered, n_lineages, top_count, top_founder = the
        lowest founder id with the largest count) and the rows by root population of the covering part.  want: an output that is not
        named goes in as NULL and comes back as None (counts is the large one)"""
        n_rows = self._rest_ind(pop, row_begin, n_rows, 2)
        pos = _arr(pos, np.uint64).ravel(); nfh = self.founder_haps(n_founder_haps)
        outs = _lineage_outs(len(pos), n_rows, int(sum(int(x) for x in nfh)) if "counts" in want else 0, self.n_pop, set(want) - {"fid"})[1:]
        self._call("founder_counts", pop, chr, row_begin, n_rows, pos, len(pos), nfh, *outs)
        return outs

    def roh_summary(self, pop, chr, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None, min_snps=0, min_bp=0, max_gap_bp=0, want_cover=True):
        """-> (n_roh, roh_bp, roh_snps, max_bp, cover): per individual of [ind_begin, +n_ind) over its qualifying runs of homozygosity among
        the SNPs [snp_begin, +n_snps) (runs are cut at the range's ends), uint32 / uint64 / uint32 / uint64 [n_ind]: their number, their
        summed length pos[j1] - pos[j0], their summed SNPs and the longest (0 without one); cover uint32 [n_snps] (None unless wanted): the
        individuals with the SNP inside a qualifying run.  A run: consecutive SNPs at which the two haplotypes agree (mutations applied),
        broken where neighbouring SNPs lie more than max_gap_bp apart; it qualifies with >= min_snps SNPs and >= min_bp base pairs (0 =
        no limit, each).  Scanned on the device from the current generation's rows"""
        n_snps = self._rest_snps(pop, chr, snp_begin, n_snps)
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        q = _roh_params(min_snps, min_bp, max_gap_bp)
        outs = _roh_outs(n_ind, n_snps, want_cover)
        self._call("roh_summary", pop, chr, snp_begin, n_snps, ind_begin, n_ind, C.byref(q), *outs)
        return outs

    def roh_segments(self, pop, chr, snp_begin=0, n_snps=None, ind_begin=0, n_ind=None, min_snps=0, min_bp=0, max_gap_bp=0):
        """-> ROH_SEGMENT_DTYPE records (st, en, ind, snp_first, n_snps, reserved), sorted by (ind, snp_first): the qualifying runs of
        roh_summary themselves, st = pos[snp_first] and en = pos[snp_first + n_snps - 1] both inclusive, ind and snp_first absolute.  A
        count call, then a fill call"""
        n_snps = self._rest_snps(pop, chr, snp_begin, n_snps)
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        q = _roh_params(min_snps, min_bp, max_gap_bp)
        return _record_list(lambda out, cap, n: self._call("roh_segments", pop, chr, snp_begin, n_snps, ind_begin, n_ind, C.byref(q), out, cap, n), ROH_SEGMENT_DTYPE)

    def ancestry_bp(self, pop, chr, row_begin=0, n_rows=None):
        """-> (bp uint64 [n_rows][n_pop], n_parts uint32 [n_rows]): the base pairs of every haplotype row covered by parts of each root
        population, and the length of the row's interval list"""
        n_rows = self._rest_ind(pop, row_begin, n_rows, 2)
        bp = np.empty((max(n_rows, 0), self.n_pop), dtype=np.uint64); n_parts = np.empty(max(n_rows, 0), dtype=np.uint32)
        self._call("ancestry_bp", pop, chr, row_begin, n_rows, bp, n_parts)
        return bp, n_parts

    def format_hap_text(self, pop, chr, snp_begin=0, n_snps=None):
        """bytes of the reference's .hap file (format_hap::write_hap) for the given SNP lines"""
        L = self._nsnp[(pop, chr)]
        n_snps = L - snp_begin if n_snps is None else n_snps
        nb = n_snps * (4 * self.pop_size(pop) + 1)
        out = np.zeros(nb, dtype=np.uint8)
        self._call("format_hap_text", pop, chr, snp_begin, n_snps, out, nb)
        return out

    def format_bed(self, pop, chr, snp_begin=0, n_snps=None):
        L = self._nsnp[(pop, chr)]
        n_snps = L - snp_begin if n_snps is None else n_snps
        nb = n_snps * ((self.pop_size(pop) + 3) // 4)
        out = np.zeros(nb, dtype=np.uint8)
        self._call("format_bed", pop, chr, snp_begin, n_snps, out, nb)
        return out

    def format_vcf_gt(self, pop, chr, snp_begin=0, n_snps=None):
        """sample columns ("\\ta|b" per individual + newline) of the reference's VCF data lines (format_vcf::write_vcf_file)"""
        L = self._nsnp[(pop, chr)]
        n_snps = L - snp_begin if n_snps is None else n_snps
        nb = n_snps * (4 * self.pop_size(pop) + 1)
        out = np.zeros(nb, dtype=np.uint8)
        self._call("format_vcf_gt", pop, chr, snp_begin, n_snps, out, nb)
        return out

    def rank_f64(self, x):
        """CommFunc::ras_rank (zero-based, ties by index)"""
        x = _arr(x, np.float64)
        out = np.zeros(len(x), dtype=np.uint64)
        self._call("rank_f64", x, len(x), out)
        return out

    def download_plink_matrix(self, pop, chr, ind_begin=0, n_ind=None, stride_words=None):
        """matrix_plink_ped rows (bit 2*snp + hap) of ras_convert_interval_to_format_plink"""
        L = self._nsnp[(pop, chr)]
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        out = _rows_out(n_ind, words_for(2 * L), stride_words)
        self._call("download_plink_matrix", pop, chr, ind_begin, n_ind, out, out.shape[1])
        return out

    def format_ped_text(self, pop, chr, al0=None, al1=None, ind_begin=0, n_ind=None):
        """genotype columns of the reference's .ped lines (format_plink::write_ped_map; write_ped01_map when al0 is None)"""
        L = self._nsnp[(pop, chr)]
        n_ind = self._rest_ind(pop, ind_begin, n_ind)
        if al0 is not None:
            al0 = _arr(al0, np.uint8); al1 = _arr(al1, np.uint8)
            if len(al0) != L or len(al1) != L:
                raise ValueError("format_ped_text: one allele letter per SNP expected")
        nb = n_ind * (4 * L + 1)
        out = np.zeros(nb, dtype=np.uint8)
        self._call("format_ped_text", pop, chr, ind_begin, n_ind, al0, al1, out, nb)
        return out

    def download_cv(self, pop, phen, chr):
        ncv = self._ncv[(pop, phen, chr)]
        w = words_for(ncv)
        out = np.zeros((2 * self.pop_size(pop), w), dtype=np.uint64)
        self._call("download_cv", pop, phen, chr, out, w)
        return out

    def download_intervals(self, pop, chr):
        n = C.c_size_t()
        self._call("download_intervals", pop, chr, None, None, C.byref(n))
        parts = np.zeros(n.value, dtype=PART_DTYPE)
        off = np.zeros(2 * self.pop_size(pop) + 1, dtype=np.uint64)
        self._call("download_intervals", pop, chr, parts, off, C.byref(n))
        return parts, off

    def download_mutations(self, pop, chr):
        n = C.c_size_t()
        self._call("download_mutations", pop, chr, None, None, C.byref(n))
        muts = np.zeros(n.value, dtype=np.uint64)
        off = np.zeros(2 * self.pop_size(pop) + 1, dtype=np.uint64)
        self._call("download_mutations", pop, chr, muts, off, C.byref(n))
        return muts, off

    # ---- product-only entry points
    def reserve(self, pop, max_people):
        self._call("reserve", pop, max_people)

    def plane_ptr(self, pop, chr):
        """(pool pointer, unit bytes, number of haplotype slots, device pointer of the (slot, segment) -> unit table, segments per row)"""
        p = C.c_void_p(); s = C.c_size_t(); n = C.c_size_t(); t = C.c_void_p(); g = C.c_uint32()
        self._call("plane_ptr", pop, chr, C.byref(p), C.byref(s), C.byref(n), C.byref(t), C.byref(g))
        return p.value, s.value, n.value, t.value, g.value

    def stitch_totals(self):
        """(bytes written by the dense stitch, bytes of the rows of the generations produced, segments written, segments) over all reproduce calls"""
        w = C.c_ulonglong(); t = C.c_ulonglong(); sw = C.c_ulonglong(); st = C.c_ulonglong()
        self._call("stitch_totals", C.byref(w), C.byref(t), C.byref(sw), C.byref(st))
        return w.value, t.value, sw.value, st.value

    def stream(self):
        p = C.c_void_p()
        self._call("stream", C.byref(p))
        return p.value

    def last_reproduce_ms(self):
        ms = (C.c_float * 4)()
        self._call("last_reproduce_ms", ms)
        return [float(x) for x in ms]

    def sync(self):
        self._call("sync")

    def timing_totals(self):
        ms = (C.c_double * 4)(); n = C.c_ulonglong()
        self._call("timing_totals", ms, C.byref(n))
        return [float(x) for x in ms], n.value

    def set_chr_active(self, chr, active):
        self._call("set_chr_active", chr, 1 if active else 0)
        (self._chr_off.discard if active else self._chr_off.add)(chr)

    def active_chrs(self):
        """the chromosomes set_chr_active has not switched off"""
        return [k for k in range(self.nchr) if k not in self._chr_off]

    def set_dense_state(self, on):
        self._call("set_dense_state", 1 if on else 0)

    def materialize(self, pop, chr, founder_tile, row_begin=0, n_rows=None, snp_begin=0, n_snps=None, stride_words=None):
        """genotype tile from the interval state; founder_tile: uint64 [n_founder_haps][words] holding SNPs [snp_begin, +n_snps)"""
        L = self._nsnp[(pop, chr)]
        n_snps = L - snp_begin if n_snps is None else n_snps
        n_rows = self._rest_ind(pop, row_begin, n_rows, 2)
        ft = np.ascontiguousarray(founder_tile, dtype=np.uint64)
        out = _rows_out(n_rows, words_for(n_snps), stride_words)
        self._call("materialize", pop, chr, row_begin, n_rows, snp_begin, n_snps, ft, ft.shape[1], ft.shape[0], out, out.shape[1])
        return out

    def materialize_pops(self, pop, chr, founder_tiles, row_begin=0, n_rows=None, snp_begin=0, n_snps=None):
        """as materialize(), with one founder tile per root population (list of uint64 [n_founder_haps][words])"""
        L = self._nsnp[(pop, chr)]
        n_snps = L - snp_begin if n_snps is None else n_snps
        n_rows = self._rest_ind(pop, row_begin, n_rows, 2)
        tiles = [np.ascontiguousarray(t, dtype=np.uint64) for t in founder_tiles]
        w = words_for(n_snps)
        ptrs = (C.c_void_p * len(tiles))(*[t.ctypes.data for t in tiles])
        strides = (C.c_size_t * len(tiles))(*[t.shape[1] for t in tiles])
        rows = (C.c_size_t * len(tiles))(*[t.shape[0] for t in tiles])
        out = np.zeros((n_rows, w), dtype=np.uint64)
        self._call("materialize_pops", pop, chr, row_begin, n_rows, snp_begin, n_snps, ptrs, strides, rows, out, w)
        return out

    def materialize_bed(self, pop, chr, founder_tiles, snp_begin=0, n_snps=None):
        """PLINK .bed body of a SNP range from the interval state + one founder tile per root population"""
        L = self._nsnp[(pop, chr)]
        n_snps = L - snp_begin if n_snps is None else n_snps
        tiles = [np.ascontiguousarray(t, dtype=np.uint64) for t in founder_tiles]
        ptrs = (C.c_void_p * len(tiles))(*[t.ctypes.data for t in tiles])
        strides = (C.c_size_t * len(tiles))(*[t.shape[1] for t in tiles])
        rows = (C.c_size_t * len(tiles))(*[t.shape[0] for t in tiles])
        nb = n_snps * ((self.pop_size(pop) + 3) // 4)
        out = np.zeros(nb, dtype=np.uint8)
        self._call("materialize_bed", pop, chr, snp_begin, n_snps, ptrs, strides, rows, out, nb)
        return out

    def dbg_verify_planes(self, pop, chr, founder_seeds):
        """(mismatching plane words, bad parts) of the device-side full comparison plane == materialise(intervals, synthetic founders);
        founder_seeds: the gev_synth_founders seed of every ROOT population's panel (a scalar for a single-population context)"""
        seeds = np.atleast_1d(np.asarray(founder_seeds, dtype=np.uint64))
        assert len(seeds) == self.n_pop
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        self._call("dbg_verify_planes", pop, chr, seeds, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def dbg_prefilter_sweep(self, x_begin, x_end):
        out = (C.c_ulonglong * 3)()
        self._call("dbg_prefilter_sweep", int(x_begin), int(x_end), out)
        return int(out[0]), int(out[1]), int(out[2])

    def dbg_sampling_path(self):
        """the sampling kernel the context launched last: 0 none yet, 1 k_sample_batched, 2 k_mut_sample + k_rec_sample,
        3 k_rec_chain_wg, 4 k_rec_chain"""
        v = C.c_int(-1)
        self._call("dbg_sampling_path", C.byref(v))
        return int(v.value)

    def dbg_ad_path(self):
        """the A/D kernel the context launched last: 0 none yet, 1 k_ad_accumulate, 2 k_ad_accumulate_rp, 3 / 4 k_ad_accumulate_tab
        (rows staged / read directly), 5 k_ad_accumulate_wide; + 16: the wide kernel built its terms from the column counts"""
        v = C.c_int(-1)
        self._call("dbg_ad_path", C.byref(v))
        return int(v.value)

    def dbg_sim_loc_rec(self, pop, chr, seed, cap=4096):
        """one Simulation::ras_sim_loc_rec call on the device: (breakpoints, the two rand() outputs that follow)"""
        locs = np.zeros(cap, dtype=np.uint64); k = C.c_uint32(0); nx = (C.c_int * 2)()
        self._call("dbg_sim_loc_rec", pop, chr, int(seed), locs, cap, C.byref(k), nx)
        assert k.value <= cap
        return locs[:k.value].copy(), (int(nx[0]), int(nx[1]))

    def set_overlap(self, on):
        """True (default): the dense stitch overlaps later work; False: one stream, every generation waits for its stitch"""
        self._call("set_overlap", 1 if on else 0)

    def set_stitch_mode(self, mode):
        self._call("set_stitch_mode", mode)

    def set_cv_stitch_form(self, form):
        """CV-plane stitch kernel: 0 automatic (default), 1 always k_stitch_small, 2 k_stitch_small8 where it is legal"""
        self._call("set_cv_stitch_form", form)

    def dbg_cv_stitch_launches(self):
        """(launches of k_stitch_small, launches of k_stitch_small8) since the context was created"""
        out = (C.c_ulonglong * 2)()
        self._call("dbg_cv_stitch_launches", out)
        return int(out[0]), int(out[1])

    def set_track_intervals(self, on):
        self._call("set_track_intervals", 1 if on else 0)

    def export_size(self, pop, positions):
        pos = _arr(positions, np.uint64); b = C.c_size_t()
        self._call("export_size", pop, pos, len(pos), C.byref(b))
        return b.value

    def export_rows(self, pop, positions, device_ptr, nbytes):
        pos = _arr(positions, np.uint64)
        self._call("export_rows", pop, pos, len(pos), device_ptr, nbytes)

    def remove_rows(self, pop, positions):
        pos = _arr(positions, np.uint64)
        self._call("remove_rows", pop, pos, len(pos))

    def import_rows(self, pop, device_ptr, nbytes, n):
        self._call("import_rows", pop, device_ptr, nbytes, n)
