// gev_library.hip -- C-ABI (include/geneevolve_amd.h) over the HIP kernels of gev_kernels.h.
// MI355X (gfx950) only.  Host side = plumbing: argument checks, device memory, launch order.
// No CPU fallback of any kernel exists: without a GPU every compute entry point fails loudly.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC gev_library.hip -o libgeneevolve_amd.so
//
// Environment knobs: the list at gev_create in include/geneevolve_amd.h is the one the library reads.
#include <hip/hip_runtime.h>
#include <chrono>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "gev_kernels.h"
#include "gev_outputs.h"
#include "gev_snpcount.h"
#include "gev_paircount.h"
#include "gev_migrant_record.h"
#include "gev_ldcount.h"
#include "gev_traitsum.h"
#include "gev_indscore.h"
#include "gev_ibd.h"
#include "gev_identity.h"
#include "gev_lineage.h"
#include "gev_roh.h"
#include "gev_select.h"
#include "gev_pedigree.h"
#include "gev_phenotypes.h"

static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
#define HIPC(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(GEV_EDEVICE, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #expr); } while (0)
#define GEVC(expr) do { int rc_ = (expr); if (rc_ != GEV_OK) return rc_; } while (0)
#define KCHECK() HIPC(hipGetLastError())

static inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
static inline size_t round_up(size_t a, size_t b) { return ceil_div(a, b) * b; }

// Device buffers that were outgrown while kernels may still be reading them: freeing (hipFree waits for the whole device)
// would stall the host behind the running stitch, so they are parked here and released at the next point where the
// device is idle anyway (gev_sync, serialised generations, gev_destroy) or when too much has piled up.
static bool g_trace_host = getenv("GEV_TRACE_HOST") != nullptr;      // stderr: where the host spends its time inside gev_reproduce
static double host_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double g_malloc_ms = 0; static size_t g_malloc_n = 0, g_malloc_bytes = 0;   // GEV_TRACE_HOST bookkeeping
struct Graveyard {
    struct Item { void* p; size_t bytes; int device; };
    std::vector<Item> items; size_t bytes = 0;
    void park(void* p, size_t n) { int d = 0; (void)hipGetDevice(&d); items.push_back({p, n, d}); bytes += n; }
    void drain(int device, bool device_is_idle)
    {
        bool any = false;
        for (auto& it : items) any |= it.device == device;
        if (!any) return;
        int cur = 0; (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        const double t0 = host_ms();
        if (!device_is_idle) (void)hipDeviceSynchronize();
        const double t1 = host_ms(); const size_t n0 = items.size(), b0 = bytes;
        size_t w = 0;
        for (auto& it : items) { if (it.device == device) { (void)hipFree(it.p); bytes -= it.bytes; } else items[w++] = it; }
        items.resize(w);
        if (g_trace_host) fprintf(stderr, "[gev] graveyard drain: sync %.2f ms, %zu frees of %.1f MiB in %.2f ms\n", t1 - t0, n0 - w, (b0 - bytes) / 1048576.0, host_ms() - t1);
        (void)hipSetDevice(cur);
    }
};
static Graveyard g_graveyard;                 // one host thread calls the seam

static const size_t GRAVEYARD_LIMIT = (size_t)16 << 30;

// the one allocator under Dev<T>::ensure: p / bytes = the buffer and its size, need = the bytes asked for
static int dev_grow(void*& p, size_t& bytes, size_t need, hipStream_t st, bool keep, double slack)
{
    size_t want = std::max<size_t>((size_t)(need * slack), 256);
    void* q = nullptr;
    const double tm0 = host_ms();
    hipError_t e = hipMalloc(&q, want);
    g_malloc_ms += host_ms() - tm0; g_malloc_n++; g_malloc_bytes += want;
    if (e != hipSuccess && g_graveyard.bytes) {                      // out of memory with parked buffers: release them and retry
        (void)hipGetLastError();
        int d = 0; (void)hipGetDevice(&d); g_graveyard.drain(d, false);
        e = hipMalloc(&q, want);
    }
    if (e != hipSuccess && want > need) { (void)hipGetLastError(); want = std::max<size_t>(need, 256); e = hipMalloc(&q, want); }
    if (e != hipSuccess) return fail(GEV_EDEVICE, "hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
    if (p) {
        if (keep && bytes) { HIPC(hipMemcpyAsync(q, p, bytes, hipMemcpyDeviceToDevice, st)); }
        g_graveyard.park(p, bytes);        // the old buffer may still be in use on either stream
        if (g_graveyard.bytes > GRAVEYARD_LIMIT) { int d = 0; (void)hipGetDevice(&d); g_graveyard.drain(d, false); }
    }
    p = q; bytes = want;
    return GEV_OK;
}
// A device allocation of elements of type T that only grows.  ensure() takes ELEMENTS; a launch or a work-table entry takes the buffer
// itself (it converts to T*, and buf + n is pointer arithmetic on T); bytes() is for the hipMemset / hipMemcpy calls that need the size.
// DevBytes (= Dev<uint8_t>) is sized in bytes and alone has as<U>().  It is for the buffers whose content has no one element type:
//   pool, panel       genotype rows of unit_bytes() / stride bytes: kernels read them as bytes, u32 or u64 words
//   d_snpmajor        SNP-major bit rows: u64 words, unsigned long long for the transpose's atomics, u32 halves in k_materialize_tile
//   d_stage, d_tmp, d_text, d_map   scratch of whichever call uses them (rows, ranks, text, maps with their offsets)
//   d_flag            flag words of several calls: u32 flags, or one 64-bit counter
//   bp.cnt            per-row counts of a bit-plane product: u64[n] then u32[n] twice (pair counts), u32 triples (LD, trait sums)
//   bp.ld_score       u64[n] sums, then u32[n] counts
//   gef.stat          GEF_WORDS u32 status words, then {mean, var} as doubles
//   ph.res            u32 result words, then {mean, var} pairs as doubles
//   lpc.tmp           an arena compaction's copy of the entries in use: LpPart or u64 (lp_compact_arena)
//   am.sort_tmp       scratch of gev_sort_pairs, which gives its size in bytes
// A buffer of several arrays of one type is typed and its parts are buf + offset (snp.cnt, bp.ld_win, d_sel, d_cnt).
template <class T> struct Dev {
    T* p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    Dev() = default;
    Dev(const Dev&) = delete; Dev& operator=(const Dev&) = delete;
    Dev(Dev&& o) noexcept { p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    operator T*() const { return p; }
    size_t bytes() const { return cap; }                     // of the allocation
    size_t capacity() const { return cap / sizeof(T); }      // elements that fit
    int ensure(size_t count, hipStream_t st, bool keep = false, double slack = 1.0)
    {
        if (count > SIZE_MAX / sizeof(T)) return fail(GEV_EINVAL, "device buffer of %zu elements of %zu bytes: the size overflows", count, sizeof(T));
        if (count * sizeof(T) <= cap && p) return GEV_OK;
        void* q = p;
        GEVC(dev_grow(q, cap, count * sizeof(T), st, keep, slack));
        p = (T*)q;
        return GEV_OK;
    }
    template <class U, class B = T> typename std::enable_if<std::is_same<B, uint8_t>::value, U*>::type as() const { return (U*)p; }
private:
    size_t cap = 0;                                          // bytes
};
typedef Dev<uint8_t> DevBytes;
// Pinned host memory that only grows.  Asynchronous copies from or into the old buffer may be in flight when it is replaced: the
// caller names the stream that carries them (nullptr: the whole device) and the size of the new buffer
struct PinnedBuf {
    void* p = nullptr; size_t bytes = 0;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete; PinnedBuf& operator=(const PinnedBuf&) = delete;
    int ensure(size_t need, size_t want, hipStream_t drain)
    {
        if (need <= bytes) return GEV_OK;
        if (drain) HIPC(hipStreamSynchronize(drain)); else HIPC(hipDeviceSynchronize());
        if (p) (void)hipHostFree(p);
        p = nullptr; bytes = 0;
        HIPC(hipHostMalloc(&p, want, hipHostMallocDefault));
        bytes = want;
        return GEV_OK;
    }
};
// A stream and an event that their holder owns: null until create(), destroyed with the holder, and converting to the raw handle that
// every launch, record and wait takes.  Neither is copied or moved: gev_ctx, its scratch sets and PhenoState stay where they were made
template <class H, hipError_t (*Destroy)(H)> struct Handle {
    H h = nullptr;
    Handle() = default; Handle(const Handle&) = delete; Handle& operator=(const Handle&) = delete;
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> { int create(int priority) { HIPC(hipStreamCreateWithPriority(&h, hipStreamNonBlocking, priority)); return GEV_OK; } };
struct Event : Handle<hipEvent_t, hipEventDestroy> { int create(unsigned flags) { HIPC(hipEventCreateWithFlags(&h, flags)); return GEV_OK; } };

struct ChrStatic {                       // one population x one chromosome
    std::vector<u64> rbp; std::vector<double> rprob; u64 bp_dist = 0;
    std::vector<u64> mbp; std::vector<double> mrate; bool mut_set = false;
    std::vector<u64> pos;                // Legend.pos
    Dev<GevThr> d_rthr, d_mthr; Dev<u64> d_rbp, d_mbp, d_pos; Dev<u32> d_coarse;
    size_t L = 0, stride = 0;            // bytes of a whole genotype row in flat (host-side / staging) layouts, multiple of 128
    u32 nseg = 1, seg_shift = 9;         // the device keeps a row as nseg segments of 2^seg_shift 16-byte chunks (gev_kernels.h, PoolWork)
    size_t unit_bytes() const { return (size_t)16 << seg_shift; }
    size_t pitch() const { return (size_t)nseg * unit_bytes(); }      // founder rows: row r = units r*nseg .. r*nseg+nseg-1 = a flat row of this pitch
    u32 idx_lo = 0, idx_hi = 0;          // loci inside [bp0, bp_end)
    u32 r_amax = 0, m_amax = 0;
    size_t founder_rows = 0;
    DevBytes panel; size_t panel_rows = 0; // read-only founder panel of this ROOT population, flat rows of `stride` bytes (gev_*_founder_panel): immigrants' rows are rebuilt from it
};
struct CvStatic {                        // one population x phenotype x chromosome
    std::vector<u64> bp; std::vector<double> a, d; double vd = 0; bool set = false;
    std::vector<u32> col_of_icv;         // file index -> column in the sorted CV plane
    std::vector<u32> icv_of_col;
    Dev<u64> d_pos_sorted, d_pos_file; Dev<u32> d_col_of_icv, d_icv_of_col, d_counts; Dev<double> d_a, d_d, d_frq, d_tab; Dev<uint16_t> d_partial; Dev<const double*> d_aptr, d_dptr;
    u32 C = 0, sub_w32 = 0, stride_w32 = 0;
    u32 idx_lo = 0, idx_hi = 0;
    size_t founder_rows = 0;
    bool frq_valid = false;
    bool cols_sorted = false;            // file order == position order (col_of_icv is the identity)
};
struct ChrState {
    // genotype rows: one pool of 4 * cap_people rows (two generations' worth); slot s of the current generation is pool row
    // phys[pcur][s] (gev_kernels.h, PoolWork).  phys has THREE buffers: the stitch of generation g (stream_big) still reads
    // phys of g-1 and g while the small work of g+1 writes the next one.
    DevBytes pool; Dev<u32> phys[3], live, freel, pctr; Dev<StitchItem> items[2]; u32 pool_stamp = 0;
    // the free list of the pool is rebuilt (mark + collect) only when it runs low: valid = built for the current table lineage,
    // n_free / cursor = its length and how much of it has been handed out (from the last generation's status block)
    bool pool_list_valid = false, pool_force_rebuild = false; u32 pool_n_free = 0, pool_cursor = 0, pool_last_taken = 0;
    unsigned long long pool_rebuilds = 0;
    // Sparse state (mutation lists, ancestry interval lists) in TWO forms, each derived from the other on demand:
    //   pieces (gev_lists.h): what Simulation::reproduce reads and writes -- per-range pieces shared between parent and offspring
    //   CSR (moff/mpos, poff/parts of buffer P.cur): what everything else reads (downloads, output, migration, plane-less assembly)
    // csr_valid / lp.valid say which of them describe the current generation (at least one does).
    Dev<u32> moff[2], poff[2]; Dev<u64> mpos[2]; Dev<gev_part> parts[2];
    size_t mut_total[2] = {0, 0}, parts_total[2] = {0, 0};   // list sizes of the two CSR buffers
    bool csr_valid = true;
    struct LpState {
        Dev<uint2> ptab[2], mtab[2]; Dev<LpPart> parena; Dev<u64> marena; Dev<u32> ctr, items;      // tables [P.cur] = current generation; ctr: {interval entries, mutation entries appended by an import, overflow flags}
        u32 p_used = 0, m_used = 0;                          // arena cursors (entries)
        u32 p_last = 0, m_last = 0;                          // what the last generation appended
        u32 nseg = 0, lgw = 0;
        bool valid = false, grow_p = false, grow_m = false;
        unsigned long long imports = 0, compactions = 0;     // rebuilds from whole lists (first use, after a CSR-side change); arena compactions
    } lp;
};
struct PopState {
    std::vector<ChrStatic> cs;                         // [chr]
    std::vector<std::vector<CvStatic>> cv;             // [phen][chr]
    std::vector<ChrState> st;                          // [chr]
    std::vector<std::vector<std::array<Dev<u32>, 2>>> cvp; // [phen][chr][2]
    Dev<ChrDev> d_chrdev;
    Dev<uint8_t> d_sex[2];                                 // Human::sex of the individuals (1 male, 2 female), physical row order, [cur]: what Simulation::random_mate reads (gev_random_mate)
    int cur = 0, pcur = 0;                             // current buffer of the double-buffered lists / of phys[3]
    size_t n_people = 0, cap_people = 0;
    // After a cross-GPU migration the individuals of the current generation are not moved physically:
    // `logical[i]` = physical individual index of logical position i (empty = identity).  The next
    // gev_reproduce maps parent positions through it and writes a dense generation again; anything
    // else that needs the dense order calls materialize_order() first.
    std::vector<u32> logical;
    size_t n_phys = 0;
    bool finalized = false, gen0 = false;
    // bumped whenever logical positions stop naming the physical rows they named (a new generation, a migration, rows removed or
    // imported, the order materialised): couples gev_random_mate left on the device are only valid for the epoch they were made in
    unsigned long long layout_epoch = 0;
    // gev_compute_selection: phenotypes of the current generation (gev_scale_ad_compute_gef writes column p; phen_ok[p] = written since the
    // individuals last changed) and Human::mating_value / selection_value / selection_value_func, [3][n_people] (sel_ok = computed since
    // then); [sbuf] is current, gev_migrate gathers into the other one.  d_sv0 = {_gen0_SV_mean, _gen0_SV_var} (sv0_ok: known)
    Dev<double> d_phen[2], d_sel[2], d_sv0;
    int sbuf = 0;
    std::vector<uint8_t> phen_ok;
    bool sel_ok = false, sv0_ok = false;
    void drop_selection() { std::fill(phen_ok.begin(), phen_ok.end(), 0); sel_ok = false; comp_ok = false; cs_ok = false; }
    // gev_set_track_pedigree: the seven ID fields of the current generation (gev_pedigree.h), planes of ids_stride[ibuf] rows indexed by
    // PHYSICAL row; [ibuf] is current, a generation in flight / gev_migrate / a materialised order write the other one.  ids_ok: they
    // describe the current individuals (dropped by gev_remove_rows / gev_import_rows, restored by gev_upload_pedigree)
    Dev<int64_t> d_ids[2]; size_t ids_stride[2] = {0, 0};
    int ibuf = 0;
    bool ids_ok = false;
    // gev_generation_phenotypes (gev_phenotypes.h).  d_cidx[ibuf]: the couple index of every child of the generation just published,
    // cs_seed / cs_ncouples its seed_reproduce and the length of its couples list (cs_ok: until the rows change) -- what the family
    // effect of Simulation::reproduce is drawn from.  d_comp[cbuf]: [nphen][7][n_people] A D G C E F P of the current individuals
    // (comp_ok; they follow gev_migrate).  d_prev: the saved record [nphen][2][prev_n] (phen, parental_effect).  ad0: host copies of
    // _var_a_gen0 / _var_d_gen0 per phenotype
    Dev<u32> d_cidx[2]; Dev<double> d_comp[2], d_prev;
    int cbuf = 0;
    bool cs_ok = false, comp_ok = false, prev_ok = false, ad0_ok = false;
    u32 cs_seed = 0; size_t cs_ncouples = 0, prev_n = 0;
    std::vector<double> ad0;
};

// gev_ctx::Scratch::ev, the events of a scratch set that only order device work against device work.  FORK .. FORKED: joins of the attempt's side streams; RECS: sampling records complete on S (for X); POOL: unit table, work list and their counters complete on X
enum DevEvent { EV_FORK, EV_AUX, EV_LISTS, EV_FORKED, EV_RECS, EV_POOL, EV_SMALL_DONE, EV_STITCH_DONE, EV_SAMPLED, EV_CHAIN, EV_TAB, N_DEV_EVENTS };
struct gev_ctx {
    // The context owns every HIP handle it uses (Stream, Event, Dev, PinnedBuf).  ~gev_ctx waits for the streams and drains the graveyard;
    // the members then go in reverse declaration order.  The streams are declared FIRST, so they are destroyed LAST: after every Dev has
    // been freed and every event destroyed.  They are named once as a set, in creation order (gev_create), for ~gev_ctx and gev_sync
    Stream streams[5];
    Stream &stream = streams[0], &stream_samp = streams[1], &stream_aux = streams[2], &stream_list = streams[3], &stream_big = streams[4];
    ~gev_ctx()                              // also of a context gev_create gave up on (null handles); work may be in flight: a pending generation, a head start
    {
        (void)hipSetDevice(device);
        for (Stream& s : streams) if (s) (void)hipStreamSynchronize(s);
        if (g_graveyard.bytes) g_graveyard.drain(device, false);
    }
    int device = 0, n_pop = 0, nchr = 0, nphen = 0;
    u32 rp_bits = 0;
    bool ad_effects_shared = false;         // every root population has the same CV effects bit for bit (check_multipop): A/D uses the one-population term table
    bool multipop_ready = false;            // check_multipop has run for the current static inputs (ad_effects_shared, d_aptr / d_dptr are valid); setters clear it
    float last_ms[4] = {0, 0, 0, 0};
    bool track_intervals = true;
    bool track_pedigree = false;            // gev_set_track_pedigree
    std::vector<PopState> pop;
    Dev<GevRngTables> d_tables;
    // per-generation scratch: two sets, because the dense stitch of generation g (stream_big) still reads set g%2
    // while sampling / sparse state of generation g+1 (stream) fill the other one
    struct Scratch {
        Dev<u32> father, mother, mutseeds, globvals /* [2 + T] ras_glob_seed() values drawn on the device: mate seed, reproduce seed, mutation seeds */, seed_pat, seed_mat, k, bk_off, bk_idx, nmut, nm_off, status,
                 globblk /* rejection counts of this set's ras_glob_seed() draws (enqueue_glob) */;
        Dev<u64> bk, nm_pos; Dev<uint8_t> start, nm_side, sex; Dev<ChrWork> chrwork; Dev<CvWork> cvwork;
        std::vector<uint8_t> chrwork_shadow, cvwork_shadow;     // what the device copies of the tables hold (upload_table_cached)
        unsigned n_chrwork = 0, n_cvwork = 0; float sampling_ms_saved = -1;
        size_t nseg_max = 1, cv_used_max = 0; u32 cv_max = 0;    // launch shapes of the generation (enqueue_tables)
        bool pool_rebuild = false;                                                            // this attempt rebuilds the free list of the segment pool
        bool cv_count_fused = false;                                                          // k_stitch_small also counts the alleles per CV column (every grid <= 1024 columns)
        bool cv_lanes8 = false;                                                               // every CV plane of the launch has the shape k_stitch_small8 takes (enqueue_tables)
        Event ev[N_DEV_EVENTS], t[6];                    // device-only events, by DevEvent; kernel timings (harvest_timing)
        Event ev_status;                                 // the generation's status block (and A/D results) have arrived on the host
        bool timing_pending = false, stitch_pending = false;
        Event tc[3];                                     // GEV_TRACE_HOST alone: start of the attempt's main stream, A/D done, lists joined
        double th_enq = 0;
        // A head start: the sampling of this set's NEXT generation, enqueued on the head-start stream before its begin call -- by
        // gev_presample for exactly these inputs, or by gev_set_generation_chain's generation in flight (seeds drawn from the predicted
        // engine state, c->chain_state) for the same population and size.  dropped: void (a redo of the generation in flight changed the
        // record capacities, a setter the maps) though its kernels may still run; gev_presample_sex samples again from the retained inputs
        struct HeadStart { enum Kind { NONE, PRESAMPLE, CHAIN } kind = NONE; bool dropped = false, has_mut = false; int pop = -1; size_t n_people = 0; u32 seed = 0 /* seed_reproduce (PRESAMPLE) */; } hs;
        // gev_random_mate: father / mother of this set hold the couples of the next gev_reproduce (couples == NULL) of mate_pop
        bool mated = false, mate_assort = false; int mate_pop = -1; size_t mate_n = 0; unsigned long long mate_epoch = 0;
        Dev<u32> cidx;              // gev_set_track_pedigree: the couple index of every child of a couples list the host passed
    } sc[2];
    unsigned gen_counter = 0;
    std::vector<uint8_t> chr_active;        // 0: chromosome held by another context (gev_set_chr_active); sampling chain only
    bool any_inactive = false;
    bool migrant_rows = true;               // false (gev_set_migrant_rows): gev_export_rows packs no genotype rows, gev_import_rows rebuilds them from the founder panels
    Dev<u32> d_poff; Dev<uint2> d_prange;                  // rebuild of immigrants' rows: PanelRef per root population, offsets of the rows' parts in the payload
    bool dense = true;                      // false: no resident genotype planes (gev_set_dense_state); lists + CV planes only, output by gev_materialize
    bool planes_pending = false;            // a stitch may still be writing the current planes (stream_big)
    Event ev_planes;                        // recorded after the most recent stitch
    double ms_sum[4] = {0, 0, 0, 0}; unsigned long long ms_count = 0;
    size_t bk_ovf_cap = 1 << 16, nm_ovf_cap = 1 << 16;       // overflow regions of the breakpoint / new-mutation records (GEV_OVF_CAP: initial size, tests force redos with a tiny one)
    int chain_draws = -1;                                    // gev_set_generation_chain: ras_glob_seed() draws the host makes between two generations (-1: unknown, no head start)
    bool chain_valid = false; u32 chain_state = 0;           // glob_generator state the queued head start assumed for the next gev_generation_begin
    unsigned long long redo_count = 0;                       // generations that were enqueued again with larger buffers (gev_redo_count)
    unsigned long long redo_pool_count = 0;                  // ... of which because the free list of the unit pool ran out (gev_dbg_pool_stats)
    PinnedBuf h_stage;                                       // pinned host staging
    PinnedBuf h_seeds;                                       // pinned copy of the mutation seeds handed to gev_presample
    // pinned A/D result cache, two buffers: [(gen_counter + 1) & 1] holds the PUBLISHED generation's values, the generation in flight
    // fills the other one -- gev_compute_ad may therefore be served between gev_generation_begin and _end (the host hands the next
    // generation over first and reads the last one's A/D while the device works)
    PinnedBuf h_ad2[2]; bool ad_dom_zero2[2] = {false, false};
    int ad_cached_pop = -1;                                  // population whose current-generation A/D sits in h_ad
    int ad_host_set_pop = -1;                                // population whose raw A/D totals on the device were supplied by gev_set_ad (locus-split: all-reduced)
    bool eager_ad = true;                                    // compute A/D inside gev_reproduce (same enqueue, same sync)
    int stitch_mode = 0;           // 0 = work-list form (production, k_stitch_segments), 1 = gamete-major (k_stitch_rows)
    int cv_stitch_form = 0;        // CV-plane stitch (gev_set_cv_stitch_form): 0 = by the planes' shape, 1 = always k_stitch_small, 2 = k_stitch_small8 where it is legal
    unsigned long long cv_stitch_launches[2] = {0, 0};      // launches of k_stitch_small / k_stitch_small8 (gev_dbg_cv_stitch_launches)
    bool sample_batched = true;               // K1-K3 as eight tasks per wave (gev_sample8.h); GEV_SAMPLE_BATCHED=0: one task per wave
    bool chain_wg = true;                     // no mutation map: a workgroup per link of the gamete chain (k_rec_chain_wg); GEV_CHAIN_WG=0: the one-wave form (k_rec_chain)
    int ad_path = 0;                          // the A/D kernel launched last (gev_dbg_ad_path): AD_PATH_*, + AD_PATH_FROM_COUNTS when it built its terms from the column counts itself
    int sampling_path = 0;                    // the sampling kernel launched last (gev_dbg_sampling_path): 0 none yet, 1 k_sample_batched, 2 k_mut_sample + k_rec_sample, 3 k_rec_chain_wg, 4 k_rec_chain
    size_t list_headroom = 48;                // spare list entries per haplotype row when a list buffer is (re)allocated; GEV_LIST_HEADROOM=0 (tests): just what is live, every generation overflows, grows and is enqueued again
    bool ad_no_shared = false;                // GEV_AD_SHARED=0 (tests): force the per-haplotype effect lookup
    bool ad_no_rp = false;                    // GEV_AD_RP_FAST=0 (tests): several root populations without the piecewise kernel
    size_t table_ring_min = (size_t)(256 << 10);   // smallest pinned ring of the table uploads; GEV_TABLE_RING_BYTES (tests shrink it to force wrap-arounds)
    bool serialize = false;        // gev_set_overlap(0) / GEV_OVERLAP=0: wait for every stitch, everything on the main stream (kernel timings without interference)
    u32 seg_shift = 7;             // log2(16-byte chunks per row segment): 2 KiB.  Smaller: more table entries to manage per generation; larger: more bytes copied per
                                   // crossover.  Round 3 (free list kept across generations, one thread per table entry), config 2: 128 chunks 906, 256: 845, 512: 745
                                   // generations/s; round 2 (list rebuilt and every row's entries walked by one thread every generation): 256: 370, 512: 457, 1024: 450.
                                   // A row has at most 64 segments: longer rows get larger segments (gev_set_snps).  GEV_SEG_CHUNKS=<power of two>
    bool alias_rows = true;        // crossover-free gametes share their parent's pool row instead of copying it (GEV_ALIAS_ROWS=0: copy every row)
    unsigned long long chunks_written_sum = 0, chunks_total_sum = 0, segments_written_sum = 0, segments_total_sum = 0;   // over all generations and active chromosomes (gev_stitch_totals)
    struct PendingRepro { bool active = false, has_mut = false, pre = false; int pop = 0, attempt = 0; size_t n_people = 0, n_status = 0; u32 seed = 0; u32* hstatus = nullptr; double th0 = 0, th1 = 0, th2 = 0;
                          bool fused = false /* gev_generation_begin: seeds and couples are made on the device */, has_svf = false, pool_rebuilt = false; const double* d_svf = nullptr; /* with has_svf: what the mating reads */ u32 glob_state = 0; u32* hseeds2 = nullptr; uint8_t* hsex = nullptr;
                          bool assort = false; /* gev_generation_begin_assort: couples made by gev_assort_mate, seeds of reproduce drawn from glob_state */ u32 assort_seed0 = 0; size_t am_nm = 0, am_nf = 0, am_couples = 0;
                          int cidx_mode = 0; /* the children's couple index: 0 = one child per couple, 1 = listed by the host (sc.cidx), 2 = from gev_assort_mate's offspring offsets */ size_t n_couples = 0; } pend;
    DevBytes d_snpmajor, d_text;
    size_t dbg_output_chunk = 0;   // gev_dbg_output_chunk: test cap on the units one staging pass of an output call takes (0: the byte budgets)
    Dev<u32> d_logical; Dev<gev_couple> d_couples;           // shared by the mating calls (and gev_download_pedigree): a population's logical -> physical map, the Couples_Info records made last
    // Scratch of one feature's calls, a sub-state each.  ONE rule serves them all: every call of a feature ends with a sync of its stream,
    // so one set of buffers serves all its calls; a buffer is created by the first call that needs it, nothing before it.
    struct BitProdState {   // the matrix-core products over bit planes (gev_bitprod.h) under gev_pair_genotype_counts / gev_ind_genotype_counts (gev_paircount.h), gev_ld_counts / gev_ld_scores (gev_ldcount.h) and the plane side of gev_snp_trait_sums
        Dev<u64> a, b; DevBytes cnt; Dev<u32> out;         // the planes of the two sides, the per-row counts, a sub-block's results
        Dev<u32> pair_w, ld_win; DevBytes ld_score;        // gev_ind_genotype_counts: the weights; gev_ld_scores: the windows, the scores
        int n_cu = 0;                                      // compute units of the device (bitprod_launch: the tile size), asked for by the first call
        int dbg_tiles = 0;                                 // gev_dbg_bitprod_tiles: 0 = the tile size by compute units, 1 = always 64 x 64, 2 = always 128 x 128
        unsigned long long launches[2] = {0, 0};           // product launches on small / large tiles over the context's life (bitprod_launch)
    } bp;
    struct DigitProdState { Dev<int32_t> val, acc; Dev<uint4> b; Dev<long long> out; } dp;   // gev_snp_trait_sums and gev_ind_scores (gev_digitprod.h), one set for both under the rule above: the columns (quanta, weights), their operand bytes, the i32 partials and the 64-bit sums of a block of rows
    struct SnpCountState { Dev<u32> cnt; } snp;                                               // gev_snp_genotype_counts (gev_snpcount.h): the two count vectors of a call
    struct IbdState { DevBytes out; Dev<u32> flag; Dev<gev_ibd_segment> seg; Dev<u64> planes; } ibd;   // gev_ibd_sharing / gev_ancestry_bp / gev_ibd_segments (gev_ibd.h): a sub-block's results, the flag of a bad root population, a strip's records; gev_identity_states (gev_identity.h): a sub-block's nine planes
    struct LineageState { Dev<u64> pos, tab; Dev<u32> flag, lab, counts, pop, ppop; Dev<gev_lineage_site> site, psite; } lin;   // gev_founder_at / gev_founder_counts (gev_lineage.h): the call's positions, the founder counts and their prefix sums, the flag of a bad label, a batch's labels, counts, per-population sums and site records, and the per-tile partials of the last two
    struct RohState { Dev<u64> brk; DevBytes out; Dev<u32> diff, cov; Dev<gev_roh_segment> seg; } roh;   // gev_roh_summary / gev_roh_segments (gev_roh.h): the break bit plane, the per-individual results, the cover's difference array and its scan, a pass's records
    struct ListState { Dev<u32> cnt, off; Dev<unsigned long long> tot; } list;                // the record lists of gev_ibd_segments / gev_roh_segments (count_total, fill_list): a strip's or pass's counts per item, their exclusive scan, their 64-bit sum
    struct MateState { Dev<uint8_t> flag; Dev<u32> blk, posm, posf, pickblk, globblk, stat; Dev<double> svf; } mate;   // gev_random_mate and a fused generation's mating (gev_mate.h, enqueue_mate: on the attempt's streams, which the generation's end waits for); globblk is gev_glob_seeds' alone
    struct GefState { Dev<double> io; DevBytes stat; } gef;                                   // gev_scale_ad_compute_gef: its vectors; its status words (GEF_*) and {mean, var} of e
    struct LpcState { Dev<u32> bits, cnt, wpre, len, old_off, new_off; DevBytes tmp; } lpc;   // an arena compaction of the list pieces (lp_compact_arena), which waits for its own scans
    // gev_assort_mate (gev_assort.h): scratch, the last call's result and couple arrays, test knobs
    struct AssortState {
        Dev<u32> wlo, ww, ends, start, cm, cf, om, of, males, females, rnd, scnt, soff, sfill, stgt, ssrc, kept, sorted_m, sorted_f,
                 tblk, i1, i2, pm, pf, inb, ocnt, ooff, pois, stat;
        Dev<double2> stats; Dev<double> t1, t2, mv, svf; Dev<int32_t> num; Dev<int64_t> ped; DevBytes sort_tmp;
        gev_assort_result res = {0, 0, 0, 0, 0};
        bool valid = false;                               // res / pm / pf / inb / num describe the last call
        bool narrow_window = false, short_poisson = false;
        unsigned long long n_chunks = 0, n_direct = 0, pois_reruns = 0;
    } am;
    Dev<u32> d_cvdone;
    // gev_format_info_text / gev_dbg_format_g (gev_fmt_g.h): created by the first call, nothing before it
    struct FmtState { Dev<GevFmtTables> tables; Dev<u32> lens, bsum; Dev<u64> boff; Dev<double> x; Dev<unsigned long long> cnt; bool ready = false; } fm;
    // gev_format_interval_text (gev_fmt_int.h, k_int_rows).  host[p]: the founder names of root population p as gev_set_founder_names
    // left them; everything on the device (the names' arenas and offset tables, d_names = IntNames[n_pop]) is created by the first
    // formatting call, nothing before it
    struct IntState {
        struct Names { std::vector<unsigned char> bytes; std::vector<u32> offs; bool set = false; };
        std::vector<Names> host;
        std::vector<Dev<unsigned char>> d_bytes; std::vector<Dev<u32>> d_offs;
        Dev<IntNames> d_names; Dev<uint8_t> lens; Dev<u32> bsum, flag; Dev<u64> boff; Dev<int64_t> ids;
        bool uploaded = false;
    } iv;
    // gev_generation_phenotypes (gev_phenotypes.h): scratch, the call whose result block is on its way, test knob.  streams / blk /
    // partial are also the scratch of ph_streams / ph_var under gev_scale_ad_compute_gef and gev_compute_selection (one stream)
    struct PhenoState {
        DevBytes res /* result words, then {mean, var} pairs: e, the components, raw A and D */; Dev<u32> starts, blk, globblk; Dev<double> partial, eraw, cval, shift; Dev<NrmStream> streams; Dev<PhTask> tasks;
        PinnedBuf h_res;
        Event ev;                                          // the result block has arrived in h_res; created by the first call
        bool pending = false; int pop = -1; unsigned long long epoch = 0;
        std::vector<gev_pheno_scheme> scheme; int gen_num = 0, vt_type = 1; u32 glob_state = 0;
        size_t n = 0, words = 0, n_seeds = 0;
        int cand_shift = 0;                                // candidate pairs per stream are doubled this many times (grown by a rerun)
        bool short_candidates = false;                     // test hook: start far too short
        unsigned long long reruns = 0;
    } ph;
    DevBytes d_map, d_flag, d_stage, d_tmp; Dev<u32> d_cnt, d_sums, d_cvm, d_thr32; Dev<double> d_addchr, d_domchr, d_add, d_dom;
    // per-generation work tables (gev_kernels.h: ChrWork / CvWork / AdWork) are written into a ring of pinned host memory and
    // copied to the device on the stream that uses them
    PinnedBuf h_ring; size_t h_ring_off = 0;
    Dev<AdWork> d_adwork2[2]; std::vector<uint8_t> adwork_shadow[2];
    Dev<u32> d_lp_nitems;                            // [nchr] length of each chromosome's work list of list pieces to build
    std::map<double, GevThr> thr_cache;
};
typedef gev_ctx::Scratch::HeadStart HeadStart;

// ------------------------------------------------------------------------------------------
static int scan_u32_on(hipStream_t st, Dev<u32>& sums, const u32* in, size_t n, u32* out /*n+1*/)
{
    const size_t nb = ceil_div(n + 1, SCAN_ITEMS);
    GEVC(sums.ensure(nb, st));
    hipLaunchKernelGGL(k_scan_partial, dim3((unsigned)nb), dim3(256), 0, st, in, n, sums);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, st, sums, nb);
    hipLaunchKernelGGL(k_scan_final, dim3((unsigned)nb), dim3(256), 0, st, in, n, sums, out);
    KCHECK();
    return GEV_OK;
}
static int scan_u32(gev_ctx* c, const u32* in, size_t n, u32* out /*n+1*/, u32* total_host)
{
    GEVC(scan_u32_on(c->stream, c->d_sums, in, n, out));
    if (total_host) {
        HIPC(hipMemcpyAsync(total_host, out + n, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    return GEV_OK;
}
template <class T> static int h2d(gev_ctx* c, Dev<T>& b, const void* src, size_t count)
{
    GEVC(b.ensure(std::max<size_t>(count, 1), c->stream));
    if (count) HIPC(hipMemcpyAsync(b.p, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));          // src may be a caller-owned temporary
    return GEV_OK;
}
static int make_thresholds(gev_ctx* c, const std::vector<double>& p, std::vector<GevThr>& out)
{
    out.resize(p.size());
    for (size_t i = 0; i < p.size(); i++) {
        auto it = c->thr_cache.find(p[i]);
        if (it == c->thr_cache.end()) {
            GevThr t;
            if (p[i] != p[i]) return fail(GEV_EINVAL, "probability of map row %zu is NaN", i);
            if (!gev_make_threshold(p[i], t)) return fail(GEV_EUNSUPPORTED, "threshold window wider than 2 for probability %a", p[i]);
            it = c->thr_cache.emplace(p[i], t).first;
        }
        out[i] = it->second;
    }
    return GEV_OK;
}
static int check_idx(gev_ctx* c, int pop, int chr, int phen = 0)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first");
    if (pop < 0 || pop >= c->n_pop) return fail(GEV_EINVAL, "population index %d out of range", pop);
    if (chr < 0 || chr >= c->nchr) return fail(GEV_EINVAL, "chromosome index %d out of range", chr);
    if (phen < 0 || phen >= c->nphen) return fail(GEV_EINVAL, "phenotype index %d out of range", phen);
    return GEV_OK;
}

// data of a chromosome this context does not hold / operations that move whole individuals
static int check_active(gev_ctx* c, int chr, const char* what)
{
    if (!c->chr_active[chr]) return fail(GEV_ESTATE, "%s: chromosome %d is not active on this context (gev_set_chr_active)", what, chr);
    return GEV_OK;
}
static int check_dense(gev_ctx* c, const char* what)
{
    if (!c->dense) return fail(GEV_ESTATE, "%s: this context keeps no resident genotype planes (gev_set_dense_state 0); use gev_materialize", what);
    return GEV_OK;
}
// bit-column permutation of small planes (CV grid): out column j <- in column src_col[j]
__global__ void k_permute_cols(const u32* __restrict__ in, size_t in_w32, u32* __restrict__ out, size_t out_w32, u32 used_w32,
                               const u32* __restrict__ src_col, u32 Cn, size_t n_rows)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_rows * used_w32) return;
    const size_t r = q / used_w32; const u32 w = (u32)(q % used_w32);
    u32 v = 0;
    for (u32 b = 0; b < 32; b++) {
        const u32 j = w * 32 + b;
        if (j >= Cn) break;
        const u32 s = src_col[j];
        v |= ((in[r * in_w32 + (s >> 5)] >> (s & 31)) & 1u) << b;
    }
    out[r * out_w32 + w] = v;
}
__global__ void k_fill_rp(u32* __restrict__ plane, size_t stride_w32, u32 sub_w32, u32 rp_bits, u32 pop, size_t n_rows)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 used = sub_w32 * rp_bits;
    if (q >= n_rows * used) return;
    const size_t r = q / used; const u32 w = (u32)(q % used);
    const u32 b = w / sub_w32;
    plane[r * stride_w32 + sub_w32 + w] = ((pop >> b) & 1u) ? 0xffffffffu : 0u;
}

// ------------------------------------------------------------------------------------------
extern "C" {

const char* gev_last_error(void) { return g_err.c_str(); }
const char* gev_version(void) { return "geneevolve_amd 0.1 (gfx950)"; }

int gev_create(gev_ctx** out, int device, int n_pop, int nchr, int nphen)
{
    if (!out) return fail(GEV_EINVAL, "gev_create: out is null");
    *out = nullptr;
    if (n_pop < 1 || nchr < 1 || nphen < 1) return fail(GEV_EINVAL, "gev_create: n_pop, nchr, nphen must be >= 1");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(GEV_EDEVICE, "no HIP device available (%s): this library has no CPU fallback", hipGetErrorString(e));
    if (device < 0) HIPC(hipGetDevice(&device));
    if (device >= ndev) return fail(GEV_EDEVICE, "device %d not present (%d devices)", device, ndev);
    HIPC(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPC(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(GEV_EDEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    std::unique_ptr<gev_ctx> c(new gev_ctx());
    c->device = device; c->n_pop = n_pop; c->nchr = nchr; c->nphen = nphen;
    while ((1u << c->rp_bits) < (u32)n_pop) c->rp_bits++;
    // All five streams at the greatest priority: the stitch is short -- 0.15 ms at config 2 -- and at equal priority it is through
    // before it is in anybody's way (at low priority it lingered for 0.35 ms next to the latency-bound chain: 1060 against 1370
    // generations/s).  The runtime maps streams of one priority onto four hardware queues in creation order, so the order below
    // decides which two streams share a queue.
    int prio_least = 0, prio_greatest = 0;
    HIPC(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    for (Stream& s : c->streams) GEVC(s.create(prio_greatest));     // stream, stream_samp, stream_aux, stream_list, stream_big
    // Events that only order DEVICE work against device work carry no system-scope fence (by default recording an event makes the
    // preceding kernel write the dirty L2 lines back to memory: tens of microseconds behind a kernel that wrote 50 MB, paid by
    // whatever small kernel comes next).  Only the event the host waits on before it reads the results (ev_status) keeps it.
    const unsigned dev_only = hipEventDisableTiming | hipEventDisableSystemFence, timed = hipEventDisableSystemFence;
    GEVC(c->ev_planes.create(dev_only));
    c->chr_active.assign(nchr, 1);
    for (auto& sc : c->sc) {
        for (Event& e : sc.ev) GEVC(e.create(dev_only));
        GEVC(sc.ev_status.create(hipEventDisableTiming));
        for (Event& e : sc.t) GEVC(e.create(timed));
        if (g_trace_host) for (Event& e : sc.tc) GEVC(e.create(timed));
    }
    c->pop.resize(n_pop);
    for (auto& P : c->pop) {
        P.cs.resize(nchr); P.st.resize(nchr);
        P.cv.resize(nphen); P.cvp.resize(nphen);
        for (int p = 0; p < nphen; p++) { P.cv[p].resize(nchr); P.cvp[p].resize(nchr); }
        P.phen_ok.assign(nphen, 0);
    }
    GevRngTables T; gev_build_rng_tables(T);
    GEVC(h2d(c.get(), c->d_tables, &T, 1));
    if (const char* e = getenv("GEV_OVERLAP")) c->serialize = atoi(e) == 0;
    if (const char* e = getenv("GEV_SAMPLE_BATCHED")) c->sample_batched = atoi(e) != 0;
    if (const char* e = getenv("GEV_CHAIN_WG")) c->chain_wg = atoi(e) != 0;
    if (const char* e = getenv("GEV_LIST_HEADROOM")) c->list_headroom = (size_t)atol(e);
    if (const char* e = getenv("GEV_AD_SHARED")) c->ad_no_shared = atoi(e) == 0;
    if (const char* e = getenv("GEV_AD_RP_FAST")) c->ad_no_rp = atoi(e) == 0;
    if (const char* e = getenv("GEV_TABLE_RING_BYTES")) c->table_ring_min = (size_t)atol(e);
    if (const char* e = getenv("GEV_SEG_CHUNKS")) { const int v = atoi(e); u32 sh = 0; while ((1 << (sh + 1)) <= v) sh++; if (v >= 1 && sh <= 20) c->seg_shift = sh; }
    if (const char* e = getenv("GEV_ALIAS_ROWS")) c->alias_rows = atoi(e) != 0;
    if (const char* e = getenv("GEV_OVF_CAP")) { const long v = atol(e); if (v >= 1) c->bk_ovf_cap = c->nm_ovf_cap = (size_t)v; }
    if (const char* e = getenv("GEV_STITCH_MODE")) c->stitch_mode = std::max(0, std::min(atoi(e), 1));
    *out = c.release();
    return GEV_OK;
}
void gev_destroy(gev_ctx* c) { if (c) delete c; }     // ~gev_ctx: waits for the streams, then releases everything in the order the struct sets

// ---- static inputs -----------------------------------------------------------------------
// a setter changed what check_multipop compared or tabulated (grids, map ranges, CV positions and effects, the a / d device arrays):
// the next A/D, eager A/D or migration runs it again instead of reading effect tables that may be stale or freed
static void drop_multipop(gev_ctx* c) { c->multipop_ready = false; c->ad_effects_shared = false; }
int gev_set_rmap(gev_ctx* c, int pop, int chr, const u64* bp, const double* prob, size_t R, u64 bp_dist)
{
    GEVC(check_idx(c, pop, chr));
    if (!bp || !prob || R < 2) return fail(GEV_EINVAL, "set_rmap: need >= 2 map rows");
    if (bp_dist == 0) return fail(GEV_EINVAL, "set_rmap: bp_dist_in_rmap is 0 (rand() %% 0 in the reference, src/Simulation.cpp:2990)");
    if (R > 0x7fffffffu) return fail(GEV_EINVAL, "set_rmap: too many rows");
    // dense-equivalence precondition: breakpoints bp[j] + rand()%dist must come out ascending
    for (size_t j = 0; j + 1 < R; j++)
        if (bp[j + 1] < bp[j] + bp_dist) return fail(GEV_EUNSUPPORTED, "set_rmap: map rows %zu,%zu are closer than bp_dist_in_rmap=%llu: the reference would emit unsorted breakpoints (overlapping parts), which has no dense equivalent", j, j + 1, (unsigned long long)bp_dist);
    ChrStatic& S = c->pop[pop].cs[chr];
    S.rbp.assign(bp, bp + R); S.rprob.assign(prob, prob + R); S.bp_dist = bp_dist;
    drop_multipop(c);
    std::vector<GevThr> thr;
    GEVC(make_thresholds(c, S.rprob, thr));
    S.r_amax = 0; for (const GevThr& t : thr) S.r_amax = std::max(S.r_amax, t.a_hi);
    HIPC(hipSetDevice(c->device));
    GEVC(h2d(c, S.d_rthr, thr.data(), R));
    GEVC(h2d(c, S.d_rbp, bp, R));
    c->pop[pop].finalized = false;
    return GEV_OK;
}
int gev_set_mutmap(gev_ctx* c, int pop, int chr, const u64* bp, const double* rate, size_t M)
{
    GEVC(check_idx(c, pop, chr));
    if (M && (!bp || !rate)) return fail(GEV_EINVAL, "set_mutmap: null arrays");
    if (M > 0x7fffffffu) return fail(GEV_EINVAL, "set_mutmap: too many rows");
    for (size_t i = 1; i < M; i++) {
        if (bp[i] < bp[i - 1]) return fail(GEV_EUNSUPPORTED, "set_mutmap: bp must be non-decreasing (row %zu)", i);
        if (bp[i] - bp[i - 1] >= 2147483645ull) return fail(GEV_EUNSUPPORTED, "set_mutmap: interval %zu spans >= 2^31 bp (uniform_int_distribution up-scaling branch)", i);
    }
    ChrStatic& S = c->pop[pop].cs[chr];
    S.mbp.assign(bp, bp + M); S.mrate.assign(rate, rate + M); S.mut_set = true;
    std::vector<GevThr> thr;
    GEVC(make_thresholds(c, S.mrate, thr));
    S.m_amax = 0; for (size_t i = 1; i < M; i++) S.m_amax = std::max(S.m_amax, thr[i].a_hi);
    HIPC(hipSetDevice(c->device));
    GEVC(h2d(c, S.d_mthr, thr.data(), M));
    GEVC(h2d(c, S.d_mbp, bp, M));
    c->pop[pop].finalized = false;
    return GEV_OK;
}
int gev_set_snps(gev_ctx* c, int pop, int chr, const u64* pos, size_t L)
{
    GEVC(check_idx(c, pop, chr));
    if (L && !pos) return fail(GEV_EINVAL, "set_snps: null positions");
    if (L >= 0xffffff00ull) return fail(GEV_EINVAL, "set_snps: too many loci");
    for (size_t i = 1; i < L; i++) if (pos[i] < pos[i - 1]) return fail(GEV_EUNSUPPORTED, "set_snps: positions must be non-decreasing (locus %zu)", i);
    ChrStatic& S = c->pop[pop].cs[chr];
    S.pos.assign(pos, pos + L); S.L = L;
    drop_multipop(c);
    S.panel_rows = 0;                                              // a founder panel kept for another grid is void
    S.stride = std::max<size_t>(round_up(ceil_div(L, 8), 128), 128);
    S.seg_shift = c->seg_shift;                                    // 2 KiB segments (GEV_SEG_CHUNKS) unless the row would need more than 64 of them
    while (ceil_div(S.stride / 16, (size_t)1 << S.seg_shift) > POOL_SEG_MAX) S.seg_shift++;
    while (S.seg_shift > 0 && ((size_t)1 << (S.seg_shift - 1)) >= S.stride / 16) S.seg_shift--;     // a row shorter than a segment: the smallest power-of-two unit that holds it
    S.nseg = (u32)ceil_div(S.stride / 16, (size_t)1 << S.seg_shift);
    HIPC(hipSetDevice(c->device));
    GEVC(h2d(c, S.d_pos, pos, L));
    c->pop[pop].finalized = false;
    return GEV_OK;
}
int gev_set_cvs(gev_ctx* c, int pop, int phen, int chr, const u64* bp, const double* a, const double* d, size_t C, double vd)
{
    GEVC(check_idx(c, pop, chr, phen));
    if (C && (!bp || !a || !d)) return fail(GEV_EINVAL, "set_cvs: null arrays");
    if (C > 0x7fffff00u) return fail(GEV_EINVAL, "set_cvs: too many CVs");
    if (c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first");
    CvStatic& V = c->pop[pop].cv[phen][chr];
    // the CV planes of a current generation hold its alleles at the positions they were built for (later generations inherit them
    // from their parents' planes): new effects are allowed between generations, new positions only before gev_init_gen0
    if (c->pop[pop].gen0 && V.set && (C != V.bp.size() || (C && memcmp(bp, V.bp.data(), C * sizeof(u64)))))
        return fail(GEV_EUNSUPPORTED, "set_cvs: population %d phenotype %d chromosome %d has a current generation whose CV planes hold the "
                    "alleles of the CV positions given before; new positions are only accepted before gev_init_gen0", pop, phen, chr);
    drop_multipop(c);
    V.bp.assign(bp, bp + C); V.a.assign(a, a + C); V.d.assign(d, d + C); V.vd = vd; V.C = (u32)C; V.set = true;
    // sorted column order (stable: equal positions keep file order)
    V.icv_of_col.resize(C);
    for (u32 i = 0; i < C; i++) V.icv_of_col[i] = i;
    std::stable_sort(V.icv_of_col.begin(), V.icv_of_col.end(), [&](u32 x, u32 y) { return V.bp[x] < V.bp[y]; });
    V.col_of_icv.resize(C);
    for (u32 j = 0; j < C; j++) V.col_of_icv[V.icv_of_col[j]] = j;
    V.cols_sorted = true;
    for (u32 j = 0; j < C; j++) V.cols_sorted &= V.col_of_icv[j] == j;
    std::vector<u64> sorted(C);
    for (u32 j = 0; j < C; j++) sorted[j] = V.bp[V.icv_of_col[j]];
    V.sub_w32 = (u32)std::max<size_t>(ceil_div(C, 32), 1);
    V.stride_w32 = (u32)round_up((size_t)V.sub_w32 * (1 + c->rp_bits), 4);      // sub-rows: resolved alleles, root-population bits
    HIPC(hipSetDevice(c->device));
    GEVC(h2d(c, V.d_pos_sorted, sorted.data(), C));
    GEVC(h2d(c, V.d_pos_file, V.bp.data(), C));
    GEVC(h2d(c, V.d_col_of_icv, V.col_of_icv.data(), C));
    GEVC(h2d(c, V.d_icv_of_col, V.icv_of_col.data(), C));
    GEVC(h2d(c, V.d_a, a, C));
    GEVC(h2d(c, V.d_d, d, C));
    GEVC(V.d_frq.ensure(std::max<size_t>(C, 1), c->stream));
    GEVC(V.d_counts.ensure(std::max<size_t>(C, 1), c->stream));
    HIPC(hipMemsetAsync(V.d_counts.p, 0, std::max<size_t>(C, 1) * sizeof(u32), c->stream));     // k_cv_count adds into them, k_cv_table / k_cv_freq consume and clear them
    V.frq_valid = false;
    c->ad_cached_pop = c->ad_host_set_pop = -1;
    c->pop[pop].finalized = false;
    return GEV_OK;
}

static int wait_planes(gev_ctx* c);
// pool descriptor of (population, chromosome); `alt` = the phys buffer a new generation / new slots are written to
static PoolWork pool_work(const gev_ctx* c, PopState& P, int chr, int alt)
{
    ChrState& cs = P.st[chr];
    PoolWork pw{};
    const ChrStatic& S = P.cs[chr];
    pw.pool = cs.pool.as<uint8_t>(); pw.phys_cur = cs.phys[P.pcur]; pw.phys_alt = cs.phys[alt];
    pw.live = cs.live; pw.freel = cs.freel; pw.pctr = cs.pctr;
    pw.nseg = S.nseg; pw.seg_shift = S.seg_shift;
    pw.pool_units = (u32)(4 * P.cap_people * S.nseg); pw.alias = c->alias_rows ? 1u : 0u;
    pw.items = cs.items[P.cur ^ 1]; pw.items_cap = (u32)(2 * P.cap_people * S.nseg);
    pw.stamp = cs.pool_stamp;                             // (pool_new_stamp before a rebuild of the free list)
    return pw;
}
static void pool_new_stamp(ChrState& cs) { if (++cs.pool_stamp == 0) cs.pool_stamp = 1; }   // (a stale mark of 2^32 rebuilds ago could only keep a free unit out of one free list)
// read access to the current generation's rows / a flat buffer of whole rows, for the kernels that move or read rows
static RowMap row_map(const PopState& P, int chr)
{
    const ChrStatic& S = P.cs[chr]; const ChrState& cs = P.st[chr];
    return RowMap{cs.pool.as<uint8_t>(), cs.phys[P.pcur], S.nseg, S.seg_shift};
}
static RowRef pool_rows(const PopState& P, int chr, const u32* table)
{
    const ChrStatic& S = P.cs[chr];
    return RowRef{P.st[chr].pool.as<uint8_t>(), table, 0, S.nseg, S.seg_shift};
}
static RowRef flat_rows(void* base, size_t stride_bytes) { return RowRef{(uint8_t*)base, nullptr, stride_bytes / 16, 1, 0}; }
// free rows of the pool given the slots that are in use (the kernels of gev_reproduce do the same from the work table)
static int pool_free_list(const PoolWork& pw, size_t n_slots, hipStream_t st)
{
    const unsigned blocks = (unsigned)std::min<size_t>(ceil_div(std::max<size_t>(pw.pool_units, 1), 256), 1024);
    hipLaunchKernelGGL(k_pool_mark, dim3(blocks), dim3(256), 0, st, pw, n_slots);
    hipLaunchKernelGGL(k_pool_collect, dim3(blocks), dim3(256), 0, st, pw);
    KCHECK();
    return GEV_OK;
}
// fresh rows for slots [slot0, slot0 + n) of pw.phys_alt (synchronous: migration / order-restoring paths only)
static int pool_take(const PoolWork& pw, size_t slot0, size_t n, hipStream_t st)
{
    if (!n) return GEV_OK;
    hipLaunchKernelGGL(k_pool_take, dim3((unsigned)ceil_div(n * pw.nseg, 256)), dim3(256), 0, st, pw, slot0, n, pw.pctr + 2);
    hipLaunchKernelGGL(k_pool_taken, dim3(1), dim3(64), 0, st, pw, (u32)(n * pw.nseg));
    KCHECK();
    u32 flag = 0;
    HIPC(hipMemcpyAsync(&flag, pw.pctr + 2, sizeof(u32), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (flag) return fail(GEV_EDEVICE, "genotype row pool exhausted (internal error)");
    return GEV_OK;
}
static int ensure_capacity(gev_ctx* c, int pop, size_t people)
{
    PopState& P = c->pop[pop];
    if (people <= P.cap_people) return GEV_OK;
    const size_t rows = 2 * people;
    // (row, position range) pairs of the list pieces are 32-bit work items (gev_lists.h): 2^27 haplotype rows per population
    if (rows * LP_MAXSEG > 0xffffffffull) return fail(GEV_EINVAL, "population %d: %zu individuals are more than this library holds (%llu)", pop, people, 0xffffffffull / LP_MAXSEG / 2);
    // Growth copies the CURRENT buffers (keep = true) on `stream`; the stitch that produces the current planes may still be
    // running on stream_big (gev_reproduce does not wait for it), so order the copies behind it -- otherwise the new buffer
    // would receive a half-written generation.
    GEVC(wait_planes(c));
    for (int k = 0; k < c->nchr; k++) {
        if (!c->chr_active[k]) continue;
        if (!P.cs[k].stride) return fail(GEV_ESTATE, "set_snps must precede allocation (pop %d chr %d)", pop, k);
        if (c->dense) {
            ChrState& cs = P.st[k];
            const size_t units = rows * P.cs[k].nseg;                                          // per generation
            GEVC(cs.pool.ensure(2 * units * P.cs[k].unit_bytes(), c->stream, /*keep=*/true));   // unit numbers stay valid: the pool grows at its end
            for (int b = 0; b < 3; b++) GEVC(cs.phys[b].ensure(units, c->stream, b == P.pcur));
            for (int b = 0; b < 2; b++) GEVC(cs.items[b].ensure((units + 1), c->stream));
            GEVC(cs.live.ensure(2 * units, c->stream)); GEVC(cs.freel.ensure(2 * units, c->stream));
            HIPC(hipMemsetAsync(cs.live.p, 0, cs.live.bytes(), c->stream)); cs.pool_stamp = 0;   // marks are generation stamps: start from a clean buffer
            GEVC(cs.pctr.ensure(8, c->stream));
            cs.pool_list_valid = false;                                                         // the pool grew: its new units are in no free list yet
        }
        for (int b = 0; b < 2; b++) {
            GEVC(P.st[k].moff[b].ensure((rows + 1), c->stream, b == P.cur));
            GEVC(P.st[k].poff[b].ensure((rows + 1), c->stream, b == P.cur));
        }
        for (int p = 0; p < c->nphen; p++) {
            if (!P.cv[p][k].set) return fail(GEV_ESTATE, "set_cvs must precede allocation (pop %d phen %d chr %d)", pop, p, k);
            for (int b = 0; b < 2; b++)
                GEVC(P.cvp[p][k][b].ensure(rows * P.cv[p][k].stride_w32, c->stream, b == P.cur));
        }
    }
    for (int b = 0; b < 2; b++) GEVC(P.d_sex[b].ensure(people, c->stream, b == P.cur));
    P.cap_people = people;
    return GEV_OK;
}
// Locus-split populations (BASELINE config 4: 125k individuals x 5M loci do not fit one GPU twice): a context can hold the
// genotype / CV / list state of a subset of the chromosomes only.  The rand() seed chain of Simulation::reproduce runs over
// ALL (offspring, chromosome) tasks in order (:2447-2501), so every context still evaluates the mutation-sampling chain of
// every task (maps of all chromosomes are required) but samples crossovers, tracks lists, stitches planes and accumulates
// A/D for its active chromosomes only; gev_compute_ad returns exact zeros for the others.  Needs a mutation map (without
// one the chain also depends on every crossover count: then all sampling runs everywhere).
int gev_set_chr_active(gev_ctx* c, int chr, int active)
{
    GEVC(check_idx(c, 0, chr));
    for (auto& P : c->pop) if (P.gen0) return fail(GEV_ESTATE, "set_chr_active: must precede gev_init_gen0");
    c->chr_active[chr] = active ? 1 : 0;
    drop_multipop(c);
    c->any_inactive = false;
    for (uint8_t a : c->chr_active) c->any_inactive |= !a;
    for (auto& P : c->pop) P.finalized = false;
    return GEV_OK;
}
// Populations whose genotype matrix cannot be resident (BASELINE config 5: 1M individuals x 10M loci): keep the reference's
// own state only -- ancestry intervals + mutation sets (and the small CV planes A/D needs) -- and assemble genotype tiles
// on demand with gev_materialize.  Must precede gev_init_gen0; founder SNP panels are not uploaded in this mode.
int gev_set_dense_state(gev_ctx* c, int on)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first");
    for (auto& P : c->pop) if (P.gen0) return fail(GEV_ESTATE, "set_dense_state: must precede gev_init_gen0");
    c->dense = on != 0;
    if (!c->dense) c->track_intervals = true;
    return GEV_OK;
}
int gev_reserve(gev_ctx* c, int pop, size_t max_people)
{
    GEVC(check_idx(c, pop, 0));
    HIPC(hipSetDevice(c->device));
    return ensure_capacity(c, pop, max_people);
}

int gev_upload_founders(gev_ctx* c, int pop, int chr, const u64* bits, size_t row_stride_words, size_t nhap, size_t L)
{
    if (c) GEVC(check_dense(c, "upload_founders"));
    GEVC(check_idx(c, pop, chr));
    PopState& P = c->pop[pop]; ChrStatic& S = P.cs[chr];
    if (!bits || nhap < 2 || (nhap & 1)) return fail(GEV_EINVAL, "upload_founders: need an even number (>=2) of haplotype rows");
    if (L != S.L) return fail(GEV_EINVAL, "upload_founders: L=%zu but set_snps gave %zu loci", L, S.L);
    if (row_stride_words * 64 < L) return fail(GEV_EINVAL, "upload_founders: row stride too small");
    HIPC(hipSetDevice(c->device));
    GEVC(gev_sync(c));
    GEVC(P.st[chr].pool.ensure(nhap * S.pitch(), c->stream));                       // founder haplotype r = units r*nseg ..: flat rows of pitch()
    HIPC(hipMemsetAsync(P.st[chr].pool.p, 0, nhap * S.pitch(), c->stream));
    HIPC(hipMemcpy2DAsync(P.st[chr].pool.p, S.pitch(), bits, row_stride_words * 8, ceil_div(L, 8), nhap, hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if (L % 8) {   // clear pad bits of the last byte (the contract says pad bits are zero; do not trust it)
        hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)ceil_div(nhap * (S.pitch() / 4), 256)), dim3(256), 0, c->stream,
                           P.st[chr].pool.as<u32>(), S.pitch() / 4, nhap, 0u, (u32)L);
        KCHECK();
    }
    S.founder_rows = nhap; P.gen0 = false;
    return GEV_OK;
}
int gev_synth_founders(gev_ctx* c, int pop, int chr, size_t nhap, u64 seed)
{
    if (c) GEVC(check_dense(c, "synth_founders"));
    GEVC(check_idx(c, pop, chr));
    PopState& P = c->pop[pop]; ChrStatic& S = P.cs[chr];
    if (nhap < 2 || (nhap & 1)) return fail(GEV_EINVAL, "synth_founders: need an even number of haplotypes");
    if (!S.L) return fail(GEV_ESTATE, "synth_founders: set_snps first");
    HIPC(hipSetDevice(c->device));
    GEVC(gev_sync(c));
    GEVC(P.st[chr].pool.ensure(nhap * S.pitch(), c->stream));
    HIPC(hipMemsetAsync(P.st[chr].pool.p, 0, nhap * S.pitch(), c->stream));
    GEVC(c->d_thr32.ensure(S.L, c->stream));
    hipLaunchKernelGGL(k_synth_thresholds, dim3((unsigned)ceil_div(S.L, 256)), dim3(256), 0, c->stream, c->d_thr32, S.L, seed);
    const size_t words = ceil_div(S.L, 64);
    hipLaunchKernelGGL(k_synth_rows, dim3((unsigned)ceil_div(nhap * words, 256)), dim3(256), 0, c->stream,
                       P.st[chr].pool.as<u64>(), S.pitch() / 8, nhap, S.L, c->d_thr32, seed);
    KCHECK();
    HIPC(hipStreamSynchronize(c->stream));
    S.founder_rows = nhap; P.gen0 = false;
    return GEV_OK;
}
// Founder panels kept for good (read-only, flat rows of S.stride bytes), one per ROOT population x chromosome: what
// Simulation::ras_convert_interval_to_hap_matrix reads as pops[root_population].hap_snps (src/Simulation.cpp:1204).  With them a
// context can rebuild an immigrant's genotype row from its ancestry intervals, so the migration payload carries lists only
// (gev_set_migrant_rows).  `pop` is the root population; it need not be a population this context simulates.
static int panel_prepare(gev_ctx* c, int pop, int chr, size_t nhap, const char* who)
{
    if (c) GEVC(check_dense(c, who));
    GEVC(check_idx(c, pop, chr));
    ChrStatic& S = c->pop[pop].cs[chr];
    if (nhap < 2 || (nhap & 1)) return fail(GEV_EINVAL, "%s: need an even number (>=2) of haplotype rows", who);
    if (!S.L || !S.stride) return fail(GEV_ESTATE, "%s: set_snps first", who);
    HIPC(hipSetDevice(c->device));
    GEVC(gev_sync(c));
    GEVC(S.panel.ensure(nhap * S.stride, c->stream));
    HIPC(hipMemsetAsync(S.panel.p, 0, nhap * S.stride, c->stream));
    return GEV_OK;
}
int gev_upload_founder_panel(gev_ctx* c, int pop, int chr, const u64* bits, size_t row_stride_words, size_t nhap, size_t L)
{
    GEVC(panel_prepare(c, pop, chr, nhap, "upload_founder_panel"));
    ChrStatic& S = c->pop[pop].cs[chr];
    if (!bits) return fail(GEV_EINVAL, "upload_founder_panel: null bits");
    if (L != S.L) return fail(GEV_EINVAL, "upload_founder_panel: L=%zu but set_snps gave %zu loci", L, S.L);
    if (row_stride_words * 64 < L) return fail(GEV_EINVAL, "upload_founder_panel: row stride too small");
    HIPC(hipMemcpy2DAsync(S.panel.p, S.stride, bits, row_stride_words * 8, ceil_div(L, 8), nhap, hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if (L % 8) {   // pad bits of the last byte
        hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)ceil_div(nhap * (S.stride / 4), 256)), dim3(256), 0, c->stream, S.panel.as<u32>(), S.stride / 4, nhap, 0u, (u32)L);
        KCHECK();
        HIPC(hipStreamSynchronize(c->stream));
    }
    S.panel_rows = nhap;
    return GEV_OK;
}
int gev_synth_founder_panel(gev_ctx* c, int pop, int chr, size_t nhap, u64 seed)
{
    GEVC(panel_prepare(c, pop, chr, nhap, "synth_founder_panel"));
    ChrStatic& S = c->pop[pop].cs[chr];
    GEVC(c->d_thr32.ensure(S.L, c->stream));
    hipLaunchKernelGGL(k_synth_thresholds, dim3((unsigned)ceil_div(S.L, 256)), dim3(256), 0, c->stream, c->d_thr32, S.L, seed);
    hipLaunchKernelGGL(k_synth_rows, dim3((unsigned)ceil_div(nhap * ceil_div(S.L, 64), 256)), dim3(256), 0, c->stream,
                       S.panel.as<u64>(), S.stride / 8, nhap, S.L, c->d_thr32, seed);      // the same generator as gev_synth_founders
    KCHECK();
    HIPC(hipStreamSynchronize(c->stream));
    S.panel_rows = nhap;
    return GEV_OK;
}
// 1 (default): gev_export_rows packs the migrants' genotype rows; 0: it packs none and gev_import_rows rebuilds them from the
// founder panels.  Both ends of an exchange must use the same setting (the payload's size gives a mismatch away).
int gev_set_migrant_rows(gev_ctx* c, int on)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first");
    c->migrant_rows = on != 0;
    return GEV_OK;
}
// CV founders arrive in FILE column order; the plane keeps columns sorted by position
static int cv_founders_from_tmp(gev_ctx* c, int pop, int phen, int chr, size_t nhap, size_t tmp_w32)
{
    PopState& P = c->pop[pop]; CvStatic& V = P.cv[phen][chr];
    GEVC(P.cvp[phen][chr][P.cur].ensure(nhap * V.stride_w32, c->stream));
    HIPC(hipMemsetAsync(P.cvp[phen][chr][P.cur].p, 0, nhap * V.stride_w32 * sizeof(u32), c->stream));
    if (V.C) {
        hipLaunchKernelGGL(k_permute_cols, dim3((unsigned)ceil_div(nhap * V.sub_w32, 256)), dim3(256), 0, c->stream,
                           c->d_tmp.as<u32>(), tmp_w32, P.cvp[phen][chr][P.cur], (size_t)V.stride_w32, V.sub_w32,
                           V.d_icv_of_col, V.C, nhap);
        KCHECK();
    }
    HIPC(hipStreamSynchronize(c->stream));
    c->ad_cached_pop = c->ad_host_set_pop = -1;
    V.founder_rows = nhap; P.gen0 = false;
    return GEV_OK;
}
int gev_upload_cv_founders(gev_ctx* c, int pop, int phen, int chr, const u64* bits, size_t row_stride_words, size_t nhap, size_t C)
{
    GEVC(check_idx(c, pop, chr, phen));
    CvStatic& V = c->pop[pop].cv[phen][chr];
    if (!V.set) return fail(GEV_ESTATE, "upload_cv_founders: set_cvs first");
    if (C != V.C) return fail(GEV_EINVAL, "upload_cv_founders: C=%zu but set_cvs gave %u", C, V.C);
    if (!bits || nhap < 2 || (nhap & 1) || row_stride_words * 64 < C) return fail(GEV_EINVAL, "upload_cv_founders: bad arguments");
    HIPC(hipSetDevice(c->device));
    GEVC(h2d(c, c->d_tmp, bits, nhap * row_stride_words * 8));
    return cv_founders_from_tmp(c, pop, phen, chr, nhap, row_stride_words * 2);
}
int gev_synth_cv_founders(gev_ctx* c, int pop, int phen, int chr, size_t nhap, u64 seed)
{
    GEVC(check_idx(c, pop, chr, phen));
    CvStatic& V = c->pop[pop].cv[phen][chr];
    if (!V.set) return fail(GEV_ESTATE, "synth_cv_founders: set_cvs first");
    if (nhap < 2 || (nhap & 1)) return fail(GEV_EINVAL, "synth_cv_founders: need an even number of haplotypes");
    HIPC(hipSetDevice(c->device));
    const size_t w64 = std::max<size_t>(ceil_div(V.C, 64), 1);
    GEVC(c->d_tmp.ensure(nhap * w64 * 8, c->stream));
    GEVC(c->d_thr32.ensure(std::max<size_t>(V.C, 1), c->stream));
    HIPC(hipMemsetAsync(c->d_tmp.p, 0, nhap * w64 * 8, c->stream));
    if (V.C) {
        hipLaunchKernelGGL(k_synth_thresholds, dim3((unsigned)ceil_div(V.C, 256)), dim3(256), 0, c->stream, c->d_thr32, (size_t)V.C, seed);
        hipLaunchKernelGGL(k_synth_rows, dim3((unsigned)ceil_div(nhap * w64, 256)), dim3(256), 0, c->stream,
                           c->d_tmp.as<u64>(), w64, nhap, (size_t)V.C, c->d_thr32, seed);
        KCHECK();
    }
    return cv_founders_from_tmp(c, pop, phen, chr, nhap, w64 * 2);
}

// the set's head start, if any, is void: no begin call takes it, the next one waits for its kernels (take_head_start)
static void drop_head_start(gev_ctx::Scratch& sc) { if (sc.hs.kind != HeadStart::NONE) sc.hs.dropped = true; }
// static tables that depend on several setters
static int finalize_static(gev_ctx* c, int pop)
{
    PopState& P = c->pop[pop];
    if (P.finalized) return GEV_OK;
    for (auto& sc : c->sc) drop_head_start(sc);              // maps / grids changed: a head start sampled with the old ones is void
    std::vector<ChrDev> cd(c->nchr);
    for (int k = 0; k < c->nchr; k++) {
        ChrStatic& S = P.cs[k];
        if (S.rbp.empty()) return fail(GEV_ESTATE, "population %d chromosome %d: set_rmap missing", pop, k);
        const u64 bp0 = S.rbp.front(), bpe = S.rbp.back();
        S.idx_lo = (u32)(std::lower_bound(S.pos.begin(), S.pos.end(), bp0) - S.pos.begin());
        S.idx_hi = (u32)(std::lower_bound(S.pos.begin(), S.pos.end(), bpe) - S.pos.begin());
        // coarse index over the SNP positions: buckets of 2^shift base pairs holding about eight loci each (at most 2^21 buckets)
        u64 cbase = 0; u32 cshift = 0, cn = 0;
        if (S.L) {
            cbase = S.pos.front();
            const u64 span = S.pos.back() - cbase + 1;
            while (cshift < 63 && ((span >> cshift) > std::max<u64>(S.L / 8, 1) || (span >> cshift) > (1ull << 21))) cshift++;
            cn = (u32)((span >> cshift) + 1);
            std::vector<u32> coarse(cn + 1);
            size_t at = 0;
            for (u32 j = 0; j <= cn; j++) {                      // coarse[j] = lower_bound(pos, cbase + (j << cshift)): one sweep
                const u64 x = cbase + ((u64)j << cshift);
                while (at < S.L && S.pos[at] < x) at++;
                coarse[j] = (u32)at;
            }
            GEVC(h2d(c, S.d_coarse, coarse.data(), coarse.size()));
        }
        cd[k] = ChrDev{S.d_rthr, S.d_rbp, S.d_mthr, S.d_mbp, S.bp_dist, bp0, bpe,
                       (u32)S.rbp.size(), (u32)S.mbp.size(), S.r_amax, S.m_amax, S.d_pos, (u32)S.L, (u32)c->chr_active[k],
                       S.d_coarse, cbase, cshift, cn};
        for (int p = 0; p < c->nphen; p++) {
            CvStatic& V = P.cv[p][k];
            if (!V.set) continue;
            std::vector<u64> sorted(V.C);
            for (u32 j = 0; j < V.C; j++) sorted[j] = V.bp[V.icv_of_col[j]];
            V.idx_lo = (u32)(std::lower_bound(sorted.begin(), sorted.end(), bp0) - sorted.begin());
            V.idx_hi = (u32)(std::lower_bound(sorted.begin(), sorted.end(), bpe) - sorted.begin());
        }
    }
    GEVC(h2d(c, P.d_chrdev, cd.data(), cd.size()));
    P.finalized = true;
    return GEV_OK;
}
// with several populations the dense state needs one shared coordinate system
static int check_multipop(gev_ctx* c)
{
    c->multipop_ready = false; c->ad_effects_shared = false;
    for (int pop = 1; pop < c->n_pop; pop++)
        for (int k = 0; k < c->nchr; k++) {
            if (!c->chr_active[k]) continue;
            const ChrStatic& A = c->pop[0].cs[k]; const ChrStatic& B = c->pop[pop].cs[k];
            if (A.pos != B.pos) return fail(GEV_EUNSUPPORTED, "populations 0 and %d have different SNP grids on chromosome %d", pop, k);
            if (A.rbp.front() != B.rbp.front() || A.rbp.back() != B.rbp.back()) return fail(GEV_EUNSUPPORTED, "populations 0 and %d have different map ranges on chromosome %d", pop, k);
            for (int p = 0; p < c->nphen; p++)
                if (c->pop[0].cv[p][k].bp != c->pop[pop].cv[p][k].bp) return fail(GEV_EUNSUPPORTED, "populations 0 and %d have different CV positions (phenotype %d chromosome %d)", pop, p, k);
        }
    // Root populations whose CV effects are the same arrays bit for bit (the usual multi-population run: one CV file for all): the mean
    // of two root populations' values (a0 + a1) / 2 (:2695-2696) is then (a + a) / 2 whatever the roots are, so the one-population
    // term table serves every haplotype and A/D need not look the root-population bits up
    c->ad_effects_shared = true;
    for (int pop = 1; pop < c->n_pop && c->ad_effects_shared; pop++)
        for (int p = 0; p < c->nphen && c->ad_effects_shared; p++)
            for (int k = 0; k < c->nchr; k++) {
                if (!c->chr_active[k]) continue;
                const CvStatic& A = c->pop[0].cv[p][k]; const CvStatic& B = c->pop[pop].cv[p][k];
                if (A.a.size() != B.a.size() || A.d.size() != B.d.size() || memcmp(&A.vd, &B.vd, sizeof(double)) ||
                    (A.a.size() && memcmp(A.a.data(), B.a.data(), A.a.size() * sizeof(double))) || (A.d.size() && memcmp(A.d.data(), B.d.data(), A.d.size() * sizeof(double)))) { c->ad_effects_shared = false; break; }
            }
    if (c->ad_no_shared) c->ad_effects_shared = false;      // GEV_AD_SHARED=0 (tests: force the per-haplotype lookup)
    // per (phen, chr): table of every population's a[] and d[] device arrays, stored with each population
    for (int pop = 0; pop < c->n_pop; pop++)
        for (int p = 0; p < c->nphen; p++)
            for (int k = 0; k < c->nchr; k++) {
                std::vector<const double*> ap(c->n_pop), dp(c->n_pop);
                for (int r = 0; r < c->n_pop; r++) { ap[r] = c->pop[r].cv[p][k].d_a; dp[r] = c->pop[r].cv[p][k].d_d; }
                GEVC(h2d(c, c->pop[pop].cv[p][k].d_aptr, ap.data(), ap.size()));
                GEVC(h2d(c, c->pop[pop].cv[p][k].d_dptr, dp.data(), dp.size()));
            }
    c->multipop_ready = true;
    return GEV_OK;
}

// ---- Simulation::ras_initial_human_gen0 ---------------------------------------------------
int gev_init_gen0(gev_ctx* c, int pop, size_t n_people, uint32_t seed_gen0, uint8_t* sex_out)
{
    GEVC(check_idx(c, pop, 0));
    if (n_people < 1) return fail(GEV_EINVAL, "init_gen0: n_people must be >= 1");
    if (2 * n_people >= 0xffffffffull) return fail(GEV_EINVAL, "init_gen0: too many people");
    HIPC(hipSetDevice(c->device));
    GEVC(gev_sync(c));
    PopState& P = c->pop[pop];
    GEVC(finalize_static(c, pop));
    const size_t rows = 2 * n_people;
    for (int k = 0; k < c->nchr; k++) {
        if (!c->chr_active[k]) continue;
        if (c->dense && P.cs[k].founder_rows < rows) return fail(GEV_ESTATE, "init_gen0: population %d chromosome %d has %zu founder haplotypes, %zu needed", pop, k, P.cs[k].founder_rows, rows);
        for (int p = 0; p < c->nphen; p++)
            if (P.cv[p][k].founder_rows < rows) return fail(GEV_ESTATE, "init_gen0: population %d phenotype %d chromosome %d has %zu CV founder haplotypes, %zu needed", pop, p, k, P.cv[p][k].founder_rows, rows);
    }
    GEVC(ensure_capacity(c, pop, std::max(n_people, P.cap_people)));
    for (int k = 0; k < c->nchr; k++) {
        if (!c->chr_active[k]) continue;
        ChrStatic& S = P.cs[k]; ChrState& st = P.st[k];
        if (c->dense) {                                  // founder haplotype r is pool row r
            hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)ceil_div(rows * (S.pitch() / 4), 256)), dim3(256), 0, c->stream,
                               st.pool.as<u32>(), S.pitch() / 4, rows, S.idx_lo, S.idx_hi);
            hipLaunchKernelGGL(k_iota_u32, dim3((unsigned)ceil_div(rows * S.nseg, 256)), dim3(256), 0, c->stream, st.phys[P.pcur], rows * S.nseg);
        }
        HIPC(hipMemsetAsync(st.moff[P.cur].p, 0, (rows + 1) * sizeof(u32), c->stream));
        GEVC(st.parts[P.cur].ensure(rows, c->stream));
        hipLaunchKernelGGL(k_init_parts, dim3((unsigned)ceil_div(rows + 1, 256)), dim3(256), 0, c->stream,
                           st.parts[P.cur], st.poff[P.cur], rows, S.rbp.front(), S.rbp.back(), pop);
        for (int p = 0; p < c->nphen; p++) {
            CvStatic& V = P.cv[p][k];
            hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)ceil_div(rows * V.stride_w32, 256)), dim3(256), 0, c->stream,
                               P.cvp[p][k][P.cur], (size_t)V.stride_w32, rows, V.idx_lo, V.idx_hi);
            // k_mask_rows zeroed the (still empty) root-population sub-rows too; write them now
            if (c->rp_bits)
                hipLaunchKernelGGL(k_fill_rp, dim3((unsigned)ceil_div(rows * V.sub_w32 * c->rp_bits, 256)), dim3(256), 0, c->stream,
                                   P.cvp[p][k][P.cur], (size_t)V.stride_w32, V.sub_w32, c->rp_bits, (u32)pop, rows);
            V.frq_valid = false;
        }
    }
    hipLaunchKernelGGL(k_sex_sequence, dim3(1), dim3(64), 0, c->stream, c->d_tables, (u32)seed_gen0, n_people, P.d_sex[P.cur]);
    KCHECK();
    P.ids_ok = false;
    if (c->track_pedigree) {                                 // ID = ID_Father = ... = i (:3037-3043)
        GEVC(P.d_ids[P.ibuf].ensure(PED_FIELDS * n_people, c->stream));
        P.ids_stride[P.ibuf] = n_people;
        hipLaunchKernelGGL(k_ped_gen0, dim3((unsigned)ceil_div(n_people, 256)), dim3(256), 0, c->stream, P.d_ids[P.ibuf], n_people, n_people);
        KCHECK();
        P.ids_ok = true;
    }
    if (sex_out) HIPC(hipMemcpyAsync(sex_out, P.d_sex[P.cur].p, n_people, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    for (int k = 0; k < c->nchr; k++) { P.st[k].mut_total[P.cur] = 0; P.st[k].parts_total[P.cur] = c->chr_active[k] ? rows : 0; P.st[k].pool_list_valid = false; P.st[k].csr_valid = true; P.st[k].lp.valid = false; }
    c->ad_cached_pop = c->ad_host_set_pop = -1;
    P.n_people = n_people; P.n_phys = n_people; P.logical.clear(); P.gen0 = true; P.layout_epoch++; P.drop_selection();
    return GEV_OK;
}

// ---- Simulation::reproduce ----------------------------------------------------------------
// Two HIP streams.  `stream` carries the small kernels of generation g (sampling, sparse lists,
// CV planes, gamete grouping) and the status/sex read-back the host waits for; `stream_big`
// carries the HBM-bound dense stitch, which the host does NOT wait for: gev_reproduce returns as
// soon as the small work is done, so A/D of generation g, host mating and the small work of
// generation g+1 overlap the stitch of generation g.  Order on stream_big serialises consecutive
// stitches (each reads the plane the previous one wrote); the scratch set a stitch reads (g%2)
// is not reused before that stitch has finished (stream waits on its event).
// No host round trip inside a generation: variable-length outputs go to capacity-checked buffers
// sized from the previous totals; if one was too small the buffers are grown from the exact totals
// of the count passes and the small work is enqueued again (inputs are untouched until the flip).
// where the allele counts of the CV columns are when the A/D kernels start: nowhere yet (k_cv_count counts the planes), in
// k_stitch_small's per-block partial counts (k_cv_finish adds them up), or complete in counts[] (k_cv_newmut_sum has added them
// up: k_ad_accumulate_wide computes its terms from them, no k_cv_finish)
enum { AD_COUNTS_NONE = 0, AD_COUNTS_PARTIAL = 1, AD_COUNTS_DONE = 2 };
static int enqueue_ad(gev_ctx* c, int pop, int buf, size_t n, int counts = AD_COUNTS_NONE, int hbuf = -1);
// the A/D kernel a population's static inputs select (enqueue_ad launches it; enqueue_attempt asks before it writes the CV planes)
enum { AD_PATH_NONE = 0, AD_PATH_GENERAL = 1, AD_PATH_RP = 2, AD_PATH_TAB = 3, AD_PATH_TAB_DIRECT = 4, AD_PATH_WIDE = 5, AD_PATH_FROM_COUNTS = 16 };
static int choose_ad_path(const gev_ctx* c, int pop, int* ipb_out, bool* skip_d_out);
static int prepare_eager_ad(gev_ctx* c, int pop);
static int check_not_pending(gev_ctx* c);
static int check_chain_size(size_t T);
static int population_has_mutmap(gev_ctx* c, int pop, bool& has_mut);
static int materialize_order(gev_ctx* c, int pop);
static int ensure_csr(gev_ctx* c, int pop);
extern "C" int gev_presample(gev_ctx* c, int pop, uint32_t seed_reproduce, const uint32_t* mut_seeds, size_t n_mut_seeds, size_t n_people);
static int wait_planes(gev_ctx* c)
{
    if (c->planes_pending) HIPC(hipStreamWaitEvent(c->stream, c->ev_planes, 0));
    return GEV_OK;
}
// the sampling time of the set's previous generation, read before a head start records the sampling events again (never blocks:
// that sampling is long over; the stitch of that generation may still run, its time is collected later by harvest_timing)
static int harvest_sampling_time(gev_ctx::Scratch& sc)
{
    if (!sc.timing_pending || sc.sampling_ms_saved >= 0) return GEV_OK;
    float t;
    HIPC(hipEventElapsedTime(&t, sc.t[0], sc.t[1]));
    sc.sampling_ms_saved = t;
    return GEV_OK;
}
static int harvest_timing(gev_ctx* c, gev_ctx::Scratch& sc)
{
    if (!sc.timing_pending) return GEV_OK;
    HIPC(hipEventSynchronize(sc.t[3]));
    float t; float ms[4];
    if (sc.sampling_ms_saved >= 0) { ms[0] = sc.sampling_ms_saved; sc.sampling_ms_saved = -1; }
    else { HIPC(hipEventElapsedTime(&t, sc.t[0], sc.t[1])); ms[0] = t; }
    HIPC(hipEventElapsedTime(&t, sc.t[4], sc.t[3])); ms[1] = t;
    HIPC(hipEventElapsedTime(&t, sc.t[5], sc.t[2])); ms[2] = t;
    ms[3] = ms[0] + ms[1] + ms[2];
    for (int i = 0; i < 4; i++) { c->last_ms[i] = ms[i]; c->ms_sum[i] += ms[i]; }
    c->ms_count++;
    sc.timing_pending = false;
    return GEV_OK;
}
// host table -> device buffer `dst` on stream `st`, staged through the pinned ring (the host copy must stay valid until the
// asynchronous copy has run: a slot is reused only after a wrap, which waits for the stream)
// ... unless the device copy already holds exactly these bytes (the tables of a scratch set repeat from generation to generation
// as long as no buffer moved): `shadow` = host copy of what was uploaded last
extern "C++" {      // (templates cannot have the C linkage of the block this file's functions sit in)
template <class T> static int upload_table(gev_ctx* c, Dev<T>& dst, const void* src, size_t count, hipStream_t st)
{
    GEVC(dst.ensure(std::max<size_t>(count, 1), st));
    if (!count) return GEV_OK;
    const size_t bytes = count * sizeof(T);
    const size_t need = round_up(bytes, 64);
    if (c->h_ring.bytes < 4 * need) {
        GEVC(c->h_ring.ensure(4 * need, std::max<size_t>(8 * need, c->table_ring_min), st));
        c->h_ring_off = 0;
    }
    if (c->h_ring_off + need > c->h_ring.bytes) { HIPC(hipStreamSynchronize(c->stream)); HIPC(hipStreamSynchronize(st)); c->h_ring_off = 0; }
    uint8_t* slot = (uint8_t*)c->h_ring.p + c->h_ring_off;
    memcpy(slot, src, bytes);
    HIPC(hipMemcpyAsync(dst.p, slot, bytes, hipMemcpyHostToDevice, st));
    c->h_ring_off += need;
    return GEV_OK;
}
template <class T> static int upload_table_cached(gev_ctx* c, Dev<T>& dst, std::vector<uint8_t>& shadow, const void* src, size_t count, hipStream_t st)
{
    const size_t bytes = count * sizeof(T);
    if (dst.p && shadow.size() == bytes && bytes && memcmp(shadow.data(), src, bytes) == 0) return GEV_OK;
    GEVC(upload_table(c, dst, src, count, st));
    shadow.assign((const uint8_t*)src, (const uint8_t*)src + bytes);
    return GEV_OK;
}
}   // extern "C++"
static SampleDev make_sd(gev_ctx* c, gev_ctx::Scratch& sc, size_t T)
{
    SampleDev sd;
    sd.seed_pat = sc.seed_pat; sd.seed_mat = sc.seed_mat; sd.k = sc.k;
    sd.bk_off = sc.bk_off; sd.bk = sc.bk; sd.bk_idx = sc.bk_idx; sd.start = sc.start;
    sd.nmut = sc.nmut; sd.nm_off = sc.nm_off; sd.nm_pos = sc.nm_pos;
    sd.nm_side = sc.nm_side; sd.sex = sc.sex;
    sd.father = sc.father; sd.mother = sc.mother;
    sd.bk_ovf_base = (u32)(2 * T * GEV_BK_CAP); sd.bk_ovf_cap = (u32)c->bk_ovf_cap;
    sd.nm_ovf_base = (u32)(T * GEV_NM_CAP); sd.nm_ovf_cap = (u32)c->nm_ovf_cap;
    sd.status = sc.status;
    return sd;
}
// per-generation scratch every phase needs (sizes depend on n_people only)
static int ensure_scratch(gev_ctx* c, gev_ctx::Scratch& sc, size_t n_people, bool has_mut)
{
    hipStream_t st = c->stream;
    const size_t T = n_people * (size_t)c->nchr;
    const size_t n_status = ST_TOTALS + ST_PER_CHR * (size_t)c->nchr;
    GEVC(sc.father.ensure(n_people, st)); GEVC(sc.mother.ensure(n_people, st));
    GEVC(sc.seed_pat.ensure((T + 1), st)); GEVC(sc.seed_mat.ensure(T, st));
    GEVC(sc.k.ensure(2 * T, st)); GEVC(sc.bk_off.ensure((2 * T + 1), st));
    GEVC(sc.start.ensure(2 * T, st)); GEVC(sc.sex.ensure(n_people, st));
    GEVC(sc.nmut.ensure(T, st)); GEVC(sc.nm_off.ensure((T + 1), st));
    GEVC(sc.nm_pos.ensure(2, st)); GEVC(sc.nm_side.ensure(16, st));
    GEVC(sc.status.ensure(n_status, st));
    if (has_mut) { GEVC(sc.mutseeds.ensure(T, st)); }
    return GEV_OK;
}
// Claim a scratch set for what `st` is about to write into it: the kernel times of the set's previous generation are collected
// before its events are recorded again, `st` waits for the stitch that last read the set, the buffers are sized for n_people
// offspring (0: the caller sizes what it fills).  host_may_block = false (a head start next to a generation in flight): nothing
// waits on the host -- only the sampling time, long over, is read; the stitch's is collected, and the set's own stream made to
// wait, when the set's generation claims it again
static int claim_scratch(gev_ctx* c, gev_ctx::Scratch& sc, hipStream_t st, bool host_may_block, size_t n_people, bool has_mut)
{
    if (host_may_block) GEVC(harvest_timing(c, sc)); else GEVC(harvest_sampling_time(sc));
    if (sc.stitch_pending) { HIPC(hipStreamWaitEvent(st, sc.ev[EV_STITCH_DONE], 0)); if (host_may_block) sc.stitch_pending = false; }
    if (n_people) GEVC(ensure_scratch(c, sc, n_people, has_mut));
    return GEV_OK;
}
// A begin call takes the head start in its scratch set if it is exactly the sampling the call would enqueue itself: alive, of the
// kind the call can use (NONE: an assortative generation uses neither), made for the same population, size and mutation seeds'
// presence, and for the same `key` -- seed_reproduce and the mutation seeds' values (PRESAMPLE), the engine state (CHAIN).  Taken:
// the main stream waits for it.  A head start that is NOT taken, alive or dropped, must not write into the set any more: the host
// waits for the head-start stream before the call refills the set.  Either way the set holds no head start and no couples after
static int take_head_start(gev_ctx* c, gev_ctx::Scratch& sc, HeadStart::Kind kind, int pop, size_t n_people, bool has_mut, u32 key, const uint32_t* mut_seeds, bool& taken)
{
    const HeadStart& h = sc.hs;
    taken = h.kind != HeadStart::NONE && h.kind == kind && !h.dropped && h.pop == pop && h.n_people == n_people && h.has_mut == has_mut;
    if (taken && kind == HeadStart::PRESAMPLE) taken = h.seed == key && (!has_mut || (c->h_seeds.p && memcmp(c->h_seeds.p, mut_seeds, n_people * (size_t)c->nchr * sizeof(u32)) == 0));
    if (taken && kind == HeadStart::CHAIN) taken = c->chain_valid && c->chain_state == key;
    if (h.kind != HeadStart::NONE && !taken) HIPC(hipStreamSynchronize(c->stream_samp));
    sc.hs = HeadStart(); sc.mated = false; c->chain_valid = false;
    if (taken) HIPC(hipStreamWaitEvent(c->stream, sc.ev[EV_SAMPLED], 0));     // the head start ran on its own stream
    return GEV_OK;
}
// K1-K3: crossover / mutation sampling and the rand() seed chain; depends on the seeds and n_people only, not on the couples
static int enqueue_sampling(gev_ctx* c, gev_ctx::Scratch& sc, int pop, size_t n_people, bool has_mut, u32 seed_reproduce, hipStream_t st,
                            const u32* seed_ptr = nullptr /* device copy of the reproduce seed */, const u32* mut_seeds_dev = nullptr /* default: sc.mutseeds */, bool clear_status = true)
{
    PopState& P = c->pop[pop];
    const int nchr = c->nchr;
    const size_t T = n_people * (size_t)nchr;
    const GevRngTables* Tb = c->d_tables;
    const ChrDev* chrs = P.d_chrdev;
    const size_t bk_fixed = 2 * T * GEV_BK_CAP, nm_fixed = T * GEV_NM_CAP;
    if (bk_fixed + c->bk_ovf_cap >= 0xffffffffull || nm_fixed + c->nm_ovf_cap >= 0xffffffffull) return fail(GEV_EINVAL, "reproduce: breakpoint/mutation record space exceeds 32-bit offsets");
    GEVC(sc.bk.ensure((bk_fixed + c->bk_ovf_cap), st));
    GEVC(sc.bk_idx.ensure((bk_fixed + c->bk_ovf_cap), st));
    if (has_mut) { GEVC(sc.nm_pos.ensure((nm_fixed + c->nm_ovf_cap), st)); GEVC(sc.nm_side.ensure(nm_fixed + c->nm_ovf_cap, st)); }
    const size_t n_status = ST_TOTALS + ST_PER_CHR * (size_t)nchr;
    if (clear_status) HIPC(hipMemsetAsync(sc.status.p, 0, n_status * sizeof(u32), st));
    SampleDev sd = make_sd(c, sc, T);
    const u32* mseeds = mut_seeds_dev ? mut_seeds_dev : sc.mutseeds;

    HIPC(hipEventRecord(sc.t[0], st));
    // ---- sampling: one map scan per gamete / per mutation task
    // persistent sampling workgroups.  Next to the other streams' kernels: 1792 (7 waves per SIMD: the kernels stall on dependent
    // integer chains and LDS, and more waves hide that -- +2 % at config 2) while the generation has few tasks; 768 for many tasks
    // (the 1.4 M tasks of the config-4 shard: its list and table kernels are the bound, and the sampling grid is in their way.  Next
    // to the 5 ms whole-row stitch of round 2, 384 was best; with the 0.7 ms segment stitch 768 finishes the sampling gev_presample_sex
    // waits for in 0.45 instead of 0.95 ms).  With the GPU to themselves: SAMPLE_GRID_MAX
    const unsigned shared_grid = T <= 400000 ? 1792u : 768u;
    const unsigned task_blocks = (unsigned)std::min<size_t>(ceil_div(T, 4), (c->dense && !c->serialize) ? shared_grid : (unsigned)SAMPLE_GRID_MAX);
    if (has_mut && c->sample_batched) {
        // eight tasks per wave, mutations and gametes in one kernel; the rare slow tasks are finished in place
        const unsigned batch_blocks = (unsigned)std::min<size_t>(ceil_div(ceil_div(T, SB_TASKS), 4), task_blocks);
        hipLaunchKernelGGL(k_sample_batched, dim3(batch_blocks), dim3(256), 0, st, Tb, chrs, nchr, mseeds, seed_reproduce, seed_ptr, T, sd);
        c->sampling_path = 1;
    } else if (has_mut) {
        hipLaunchKernelGGL(k_mut_sample, dim3(task_blocks), dim3(256), 0, st, Tb, chrs, nchr, mseeds, T, sd);
        hipLaunchKernelGGL(k_rec_sample, dim3(task_blocks), dim3(256), 0, st, Tb, chrs, nchr, seed_reproduce, seed_ptr, T, sd);
        c->sampling_path = 2;
    } else {
        // no mutation map: the gametes of a generation form ONE serial chain (src/Simulation.cpp:2447-2455).  A workgroup per link
        // (k_rec_chain_wg); GEV_CHAIN_WG=0: the one-wave form
        if (c->chain_wg) {
            size_t rows_all = 0;
            for (int k = 0; k < nchr; k++) rows_all += c->pop[pop].cs[k].rbp.size();
            const u32 thr_lds = rows_all <= 2048 ? (u32)rows_all : 0u;            // thresholds of all chromosomes in LDS when they fit into 32 KiB
            hipLaunchKernelGGL(k_rec_chain_wg, dim3(1), dim3(CHAIN_THREADS), (size_t)thr_lds * sizeof(GevThr), st, Tb, chrs, nchr, seed_reproduce, seed_ptr, T, sd, thr_lds);
            c->sampling_path = 3;
        } else { hipLaunchKernelGGL(k_rec_chain, dim3(1), dim3(64), 0, st, Tb, chrs, nchr, seed_reproduce, seed_ptr, T, sd); c->sampling_path = 4; }
    }
    KCHECK();
    HIPC(hipEventRecord(sc.t[1], st));
    return GEV_OK;
}
// ---- sparse state as shared pieces (gev_lists.h) -------------------------------------------------------------------------
// ranges of 2^lgw bp, at most LP_MAXSEG of them (GEV_LIST_SEGS: fewer; 1 = one piece per row and list)
static void lp_geometry(const ChrStatic& S, u32& nseg, u32& lgw)
{
    const u32 max_seg = getenv("GEV_LIST_SEGS") ? (u32)std::min(std::max(atoi(getenv("GEV_LIST_SEGS")), 1), LP_MAXSEG) : (u32)LP_MAXSEG;
    const u64 span = S.rbp.back() - S.rbp.front();
    lgw = 0;
    while ((span >> lgw) + 1 > max_seg) lgw++;
    nseg = (u32)(span >> lgw) + 1;
}
static size_t lp_arena_entries(size_t rows, size_t live, int n_active_chr, bool tight /* GEV_LIST_HEADROOM=0 */)
{
    // arena = room for the pieces of many generations (each appends a few entries per row): a tenth of the device memory, shared
    // out over the active chromosomes, at most 4096 entries per row (GEV_LIST_ARENA: entries per row); when it fills up, the
    // pieces are compacted (pieces -> whole lists -> pieces).  GEV_LIST_HEADROOM=0: just what is live (tests: every generation
    // then overflows, grows and is enqueued again)
    const size_t per_row_env = getenv("GEV_LIST_ARENA") ? (size_t)atol(getenv("GEV_LIST_ARENA")) : 0;      // (read at every call: tests set it per case)
    if (tight) return live + 16;
    size_t per_row = per_row_env;
    if (!per_row) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); total_b = (size_t)64 << 30; }
        const size_t budget = total_b / 10 / (size_t)std::max(n_active_chr, 1);                 // bytes for this chromosome's two arenas (16 + 8 bytes per entry pair)
        per_row = std::min<size_t>(std::max<size_t>(budget / (std::max<size_t>(rows, 1) * 24), 128), 4096);
    }
    return std::min<size_t>(per_row_env ? live + rows * per_row : std::max<size_t>(2 * live + 4096, rows * per_row), 0xfffffff0u);
}
// CSR of buffer P.cur -> pieces (tables of buffer P.cur, arenas restarted): first use, after a CSR-side change, compaction
static int lp_import_all(gev_ctx* c, PopState& P, int k, hipStream_t st)
{
    ChrStatic& S = P.cs[k]; ChrState& cs = P.st[k]; ChrState::LpState& lp = cs.lp;
    const size_t rows = 2 * P.n_phys;
    lp_geometry(S, lp.nseg, lp.lgw);
    const bool track = c->track_intervals;
    const size_t live_p = track ? cs.parts_total[P.cur] + rows * lp.nseg : 0, live_m = cs.mut_total[P.cur];
    if (live_p >= 0xfffffff0u || live_m >= 0xfffffff0u) return fail(GEV_EDEVICE, "list pieces: more than 2^32 list entries on one chromosome");
    const size_t tab_rows = std::max<size_t>(rows, 2 * P.cap_people);
    for (int b = 0; b < 2; b++) {
        if (track) GEVC(lp.ptab[b].ensure(tab_rows * lp.nseg, st));
        GEVC(lp.mtab[b].ensure(tab_rows * lp.nseg, st));
    }
    int n_active = 0; for (int q = 0; q < c->nchr; q++) n_active += c->chr_active[q] ? 1 : 0;
    if (track) GEVC(lp.parena.ensure(lp_arena_entries(rows, live_p, n_active, c->list_headroom == 0), st));
    GEVC(lp.marena.ensure(std::max<size_t>(lp_arena_entries(rows, live_m, n_active, c->list_headroom == 0), 16), st));
    GEVC(lp.ctr.ensure(4, st));
    HIPC(hipMemsetAsync(lp.ctr.p, 0, 4 * sizeof(u32), st));
    if (rows)
        hipLaunchKernelGGL(k_lp_import, dim3((unsigned)ceil_div(rows * LP_MAXSEG, 256)), dim3(256), 0, st,
                           track ? cs.poff[P.cur] : (const u32*)nullptr, track ? cs.parts[P.cur] : (const gev_part*)nullptr,
                           cs.moff[P.cur], cs.mpos[P.cur], (size_t)0, rows,
                           track ? lp.ptab[P.cur] : (uint2*)nullptr, lp.mtab[P.cur], lp.parena, lp.marena,
                           0u, 0u, (u32)(lp.parena.capacity()), (u32)(lp.marena.capacity()), lp.nseg, lp.lgw, (u64)S.rbp.front(),
                           lp.ctr, lp.ctr + 2);
    KCHECK();
    u32 h[4] = {0, 0, 0, 0};
    HIPC(hipMemcpyAsync(h, lp.ctr.p, sizeof h, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (h[2]) return fail(GEV_EDEVICE, "list pieces: import overflowed its arena (internal error: %u of %zu interval, %u of %zu mutation entries)", h[0], lp.parena.capacity(), h[1], lp.marena.capacity());
    lp.p_used = h[0]; lp.m_used = h[1]; lp.p_last = 0; lp.m_last = 0; lp.valid = true; lp.grow_p = lp.grow_m = false; lp.imports++;
    return GEV_OK;
}
// one arena of the current generation's pieces compacted in place, sharing kept (gev_lists.h); *used = entries in use afterwards
extern "C++" template <class E> static int lp_compact_arena(gev_ctx* c, uint2* tab, size_t n_entries, u32 extra, Dev<E>& arena, u32* used, hipStream_t st)
{
    const size_t elem_bytes = sizeof(E);            // k_lpc_copy moves entries of either kind as 64-bit words
    const size_t n_words = ceil_div(std::max<size_t>(*used, 1), 32);
    GEVC(c->lpc.bits.ensure(n_words, st)); GEVC(c->lpc.cnt.ensure((n_words + 1), st)); GEVC(c->lpc.wpre.ensure((n_words + 1), st));
    HIPC(hipMemsetAsync(c->lpc.bits.p, 0, n_words * sizeof(u32), st));
    const unsigned eb = (unsigned)ceil_div(std::max<size_t>(n_entries, 1), 256);
    hipLaunchKernelGGL(k_lpc_mark, dim3(eb), dim3(256), 0, st, (const uint2*)tab, n_entries, extra, c->lpc.bits);
    hipLaunchKernelGGL(k_lpc_popc, dim3((unsigned)ceil_div(n_words, 256)), dim3(256), 0, st, c->lpc.bits, n_words, c->lpc.cnt);
    KCHECK();
    u32 n_pieces = 0, total = 0;
    GEVC(scan_u32(c, c->lpc.cnt, n_words, c->lpc.wpre, &n_pieces));
    GEVC(c->lpc.len.ensure(((size_t)n_pieces + 1), st)); GEVC(c->lpc.old_off.ensure(((size_t)n_pieces + 1), st)); GEVC(c->lpc.new_off.ensure(((size_t)n_pieces + 2), st));
    hipLaunchKernelGGL(k_lpc_collect, dim3(eb), dim3(256), 0, st, (const uint2*)tab, n_entries, extra, c->lpc.bits, c->lpc.wpre, c->lpc.len, c->lpc.old_off);
    KCHECK();
    GEVC(scan_u32(c, c->lpc.len, n_pieces, c->lpc.new_off, &total));
    if (n_pieces) {
        GEVC(c->lpc.tmp.ensure(std::max<size_t>(total, 1) * elem_bytes, st));
        hipLaunchKernelGGL(k_lpc_copy, dim3((unsigned)ceil_div(n_pieces, 256)), dim3(256), 0, st, (const u64*)arena.p, c->lpc.tmp.as<u64>(), c->lpc.len, c->lpc.old_off, c->lpc.new_off, (size_t)n_pieces, (u32)(elem_bytes / 8));
        KCHECK();
        HIPC(hipMemcpyAsync(arena.p, c->lpc.tmp.p, (size_t)total * elem_bytes, hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_lpc_rewrite, dim3(eb), dim3(256), 0, st, tab, n_entries, extra, c->lpc.bits, c->lpc.wpre, c->lpc.new_off);
    KCHECK();
    *used = total;
    return GEV_OK;
}
static int lp_compact(gev_ctx* c, PopState& P, int k, hipStream_t st)
{
    ChrState::LpState& lp = P.st[k].lp;
    const size_t n_entries = 2 * P.n_phys * (size_t)lp.nseg;
    if (st != c->stream) HIPC(hipStreamSynchronize(st));
    if (c->track_intervals) GEVC(lp_compact_arena(c, lp.ptab[P.cur], n_entries, 1u, lp.parena, &lp.p_used, c->stream));
    GEVC(lp_compact_arena(c, lp.mtab[P.cur], n_entries, 0u, lp.marena, &lp.m_used, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    lp.compactions++;
    return GEV_OK;
}
// the CSR form of the current generation (buffer P.cur), materialised from the pieces when it is not there
static int ensure_csr(gev_ctx* c, int pop)
{
    PopState& P = c->pop[pop];
    hipStream_t st = c->stream;
    const size_t rows = 2 * P.n_phys;
    for (int k = 0; k < c->nchr; k++) {
        ChrState& cs = P.st[k]; ChrState::LpState& lp = cs.lp;
        if (!c->chr_active[k] || cs.csr_valid) continue;
        if (!lp.valid) return fail(GEV_ESTATE, "internal error: neither form of the sparse state is valid (pop %d chr %d)", pop, k);
        const bool track = c->track_intervals;
        GEVC(cs.moff[P.cur].ensure((rows + 1), st)); GEVC(cs.poff[P.cur].ensure((rows + 1), st));
        GEVC(c->d_cnt.ensure(2 * (rows + 1), st));
        u32* pcnt = c->d_cnt; u32* mcnt = pcnt + rows + 1;
        const unsigned blocks = (unsigned)ceil_div(std::max<size_t>(rows, 1) * LP_MAXSEG, 256);
        hipLaunchKernelGGL(k_lp_count, dim3(blocks), dim3(256), 0, st, track ? lp.ptab[P.cur] : (const uint2*)nullptr, lp.mtab[P.cur], lp.nseg,
                           (const u32*)nullptr, rows, track ? pcnt : (u32*)nullptr, mcnt);
        KCHECK();
        u32 tot_m = 0, tot_p = 0;
        GEVC(scan_u32(c, mcnt, rows, cs.moff[P.cur], &tot_m));
        if (track) GEVC(scan_u32(c, pcnt, rows, cs.poff[P.cur], &tot_p));
        GEVC(cs.mpos[P.cur].ensure(std::max<size_t>(tot_m, 2), st, false, 1.25));
        if (track) GEVC(cs.parts[P.cur].ensure(std::max<size_t>(tot_p, 1), st, false, 1.25));
        hipLaunchKernelGGL(k_lp_fill, dim3(blocks), dim3(256), 0, st, track ? lp.ptab[P.cur] : (const uint2*)nullptr, lp.mtab[P.cur],
                           lp.parena, lp.marena, lp.nseg, (const u32*)nullptr, rows, (u64)P.cs[k].rbp.back(),
                           cs.poff[P.cur], cs.parts[P.cur], cs.moff[P.cur], cs.mpos[P.cur]);
        KCHECK();
        HIPC(hipStreamSynchronize(st));
        cs.mut_total[P.cur] = tot_m; cs.parts_total[P.cur] = track ? tot_p : 0; cs.csr_valid = true;
    }
    return GEV_OK;
}
// a CSR-side change of the current generation (generation 0, migration, import, order restoring): the pieces no longer describe it
static void lists_changed_in_csr(gev_ctx* c, PopState& P)
{
    for (int k = 0; k < c->nchr; k++) { P.st[k].csr_valid = true; P.st[k].lp.valid = false; }
}
// K4/K6 + grouping: everything of the small work that needs the couples (parents) on top of the sampling results.
// Every kernel covers ALL active chromosomes in one launch (blockIdx.y = entry of the generation's ChrWork / CvWork table).
// work tables of the generation (one ChrWork per active chromosome, one CvWork per (phenotype, active chromosome)): list buffers
// sized, tables uploaded on `st`; the launch shapes the later pieces need are kept in the scratch set
static int enqueue_tables(gev_ctx* c, gev_ctx::Scratch& sc, int pop, size_t n_people, hipStream_t st)
{
    PopState& P = c->pop[pop];
    const int nchr = c->nchr;
    const size_t rows = 2 * n_people;
    const int cur = P.cur, alt = P.cur ^ 1;
    std::vector<ChrWork> cw; std::vector<CvWork> vw;
    // The free list of the segment pool is kept across generations (units nobody named when it was built and that were not handed
    // out since are still unnamed) and rebuilt only when what is left of it may not cover the generation: four times what the last
    // generation took, at least a quarter of a generation's segments.  Should a generation need more than is left (k_pool_fresh
    // raises FLAG_POOL), it is enqueued again behind a rebuild.
    sc.pool_rebuild = false;
    if (c->dense) for (int k = 0; k < nchr; k++) {
        if (!c->chr_active[k]) continue;
        ChrState& cs = P.st[k];
        const size_t left = cs.pool_n_free - std::min(cs.pool_cursor, cs.pool_n_free), gen_segs = 2 * n_people * P.cs[k].nseg;
        const size_t need = c->alias_rows ? std::max<size_t>(4 * (size_t)cs.pool_last_taken, gen_segs / 4) : gen_segs;
        sc.pool_rebuild |= !cs.pool_list_valid || cs.pool_force_rebuild || left < need;
    }
    if (sc.pool_rebuild) for (int k = 0; k < nchr; k++) if (c->chr_active[k]) pool_new_stamp(P.st[k]);     // the marks of the rebuild
    for (int k = 0; k < nchr; k++) {
        if (!c->chr_active[k]) continue;
        ChrStatic& S = P.cs[k]; ChrState& cs = P.st[k];
        // the parents' pieces: imported from the CSR form when that is what describes them; an arena that may not hold this
        // generation's pieces is compacted first (pieces -> CSR -> pieces: what no table names any more is dropped)
        ChrState::LpState& lp = cs.lp;
        const size_t rows_cur = 2 * P.n_phys;
        const size_t guess_p = std::max<size_t>(4 * (size_t)lp.p_last, 8 * rows), guess_m = std::max<size_t>(4 * (size_t)lp.m_last, 4 * rows);
        const bool tight = c->list_headroom == 0;
        // room the arenas must have on top of what is used: an attempt overflowed (its status block holds what it wanted to append) ...
        size_t need_p = lp.grow_p ? (size_t)lp.p_last * 5 / 4 + 1024 : 0, need_m = lp.grow_m ? (size_t)lp.m_last * 5 / 4 + 1024 : 0;
        if (lp.valid && !tight) {
            const size_t want_p = c->track_intervals ? std::max(need_p, guess_p) : 0, want_m = std::max(need_m, guess_m);
            const bool full_p = c->track_intervals && lp.p_used + want_p > lp.parena.capacity();
            const bool full_m = lp.m_used + want_m > lp.marena.capacity();
            if (full_p || full_m) {                           // drop the pieces nobody names any more; should that not make room, the arena grows below
                GEVC(lp_compact(c, P, k, st));
                need_p = want_p; need_m = want_m;
            }
        }
        if (!lp.valid) {
            GEVC(lp_import_all(c, P, k, st));
            if (!tight) { need_p = c->track_intervals ? guess_p : 0; need_m = guess_m; }     // ... or a fresh import has to leave room for this generation
        }
        if (need_p && lp.p_used + need_p > lp.parena.capacity())
            GEVC(lp.parena.ensure(std::min<size_t>(lp.p_used + need_p, 0xfffffff0u), st, /*keep=*/true, tight ? 1.0 : 1.5));
        if (need_m && lp.m_used + need_m > lp.marena.capacity())
            GEVC(lp.marena.ensure(std::min<size_t>(lp.m_used + need_m, 0xfffffff0u), st, /*keep=*/true, tight ? 1.0 : 1.5));
        lp.grow_p = lp.grow_m = false;
        const size_t tab_entries = std::max<size_t>(rows, rows_cur) * lp.nseg;
        if (c->track_intervals) { GEVC(lp.ptab[alt].ensure(tab_entries, st)); }
        GEVC(lp.mtab[alt].ensure(tab_entries, st));
        ChrWork w{};
        w.lp.ptab_cur = lp.ptab[cur]; w.lp.ptab_alt = lp.ptab[alt]; w.lp.mtab_cur = lp.mtab[cur]; w.lp.mtab_alt = lp.mtab[alt];
        w.lp.parena = lp.parena; w.lp.marena = lp.marena;
        w.lp.pbase = lp.p_used; w.lp.mbase = lp.m_used;
        w.lp.pcap = (u32)std::min<size_t>(lp.parena.capacity(), 0xfffffff0u); w.lp.mcap = (u32)std::min<size_t>(lp.marena.capacity(), 0xfffffff0u);
        w.lp.nseg = lp.nseg; w.lp.lgw = lp.lgw; w.lp.track = c->track_intervals ? 1u : 0u;
        GEVC(lp.items.ensure(rows * LP_MAXSEG, st));
        GEVC(c->d_lp_nitems.ensure((size_t)nchr, st));
        w.lp.items = lp.items; w.lp.n_items = c->d_lp_nitems + k;
        w.bp0 = S.rbp.front(); w.bp_end = S.rbp.back(); w.chr = k;
        if (c->dense) {
            w.pw = pool_work(c, P, k, (P.pcur + 1) % 3); w.snp_pos = S.d_pos;
            w.stride = S.stride; w.chunks = (u32)(S.stride / 16); w.L = (u32)S.L;
        }
        cw.push_back(w);
        for (int p = 0; p < c->nphen; p++) {
            CvStatic& V = P.cv[p][k];
            GEVC(V.d_partial.ensure(ceil_div(rows, SMALL_ROWS_PER_BLOCK) * 1024, st));
            vw.emplace_back();
            CvWork& v = vw.back(); memset(&v, 0, sizeof v);     // (upload_table_cached compares the table byte for byte: the padding too)
            v.cvp_alt = P.cvp[p][k][alt]; v.cvp_cur = P.cvp[p][k][cur]; v.pos_sorted = V.d_pos_sorted; v.counts = V.d_counts; v.partial = V.d_partial;
            v.bp0 = S.rbp.front(); v.bp_end = S.rbp.back(); v.stride_w32 = V.stride_w32; v.sub_w32 = V.sub_w32; v.C = V.C; v.chr = k; v.cw = (u32)(cw.size() - 1);
        }
    }
    sc.n_chrwork = (unsigned)cw.size(); sc.n_cvwork = (unsigned)vw.size();
    sc.nseg_max = 1; sc.cv_used_max = 0; sc.cv_max = 0;
    for (const ChrWork& w : cw) sc.nseg_max = std::max<size_t>(sc.nseg_max, w.pw.nseg);
    const u32 nsub = 1 + c->rp_bits;
    sc.cv_count_fused = true;
    for (const CvWork& v : vw) { sc.cv_used_max = std::max<size_t>(sc.cv_used_max, (size_t)v.sub_w32 * nsub); sc.cv_count_fused &= v.sub_w32 <= 32; if (v.C <= SMALL_POS_LDS) sc.cv_max = std::max(sc.cv_max, v.C); }   // LDS copy of the CV grid: sized for the launch, not for the worst case (occupancy)
    // eight lanes per row (k_stitch_small8): every sub-row of every plane is made of whole, aligned 16-byte chunks and at most 32 words long
    sc.cv_lanes8 = !vw.empty();
    for (const CvWork& v : vw)
        sc.cv_lanes8 &= v.sub_w32 <= 32 && v.sub_w32 % 4 == 0 && v.stride_w32 % 4 == 0 && (uintptr_t)v.cvp_alt % 16 == 0 && (uintptr_t)v.cvp_cur % 16 == 0;
    if (sc.n_chrwork) {
        GEVC(upload_table_cached(c, sc.chrwork, sc.chrwork_shadow, cw.data(), cw.size(), st));
        GEVC(upload_table_cached(c, sc.cvwork, sc.cvwork_shadow, vw.data(), vw.size(), st));
    }
    return GEV_OK;
}
// free units of the pool = units no (slot, segment) of the parents names: needs the parents' table only, not this generation's
// sampling or couples
static int enqueue_pool_free(gev_ctx* c, gev_ctx::Scratch& sc, int pop, hipStream_t st)
{
    PopState& P = c->pop[pop];
    if (!c->dense || !sc.n_chrwork || !sc.pool_rebuild) return GEV_OK;      // (decided by enqueue_tables)
    const unsigned pool_blocks = (unsigned)std::min<size_t>(ceil_div(4 * P.cap_people * sc.nseg_max, 256), 1024);
    hipLaunchKernelGGL(k_pool_mark_tab, dim3(pool_blocks, sc.n_chrwork), dim3(256), 0, st, sc.chrwork, 2 * P.n_phys);
    hipLaunchKernelGGL(k_pool_collect_tab, dim3(pool_blocks, sc.n_chrwork), dim3(256), 0, st, sc.chrwork);
    KCHECK();
    for (int k = 0; k < c->nchr; k++) if (c->chr_active[k]) { P.st[k].pool_list_valid = true; P.st[k].pool_force_rebuild = false; P.st[k].pool_rebuilds++; }
    return GEV_OK;
}
// the counters of the unit table into the status block and the length of the stitch's work list (behind k_pool_fresh)
static int enqueue_pool_publish(gev_ctx* c, gev_ctx::Scratch& sc, size_t n_people, hipStream_t st)
{
    if (!c->dense || !sc.n_chrwork) return GEV_OK;
    SampleDev sd = make_sd(c, sc, n_people * (size_t)c->nchr);
    hipLaunchKernelGGL(k_pool_publish, dim3(1), dim3(64), 0, st, sc.chrwork, sc.n_chrwork, sd.status);
    KCHECK();
    return GEV_OK;
}
// units of the offspring rows (segments with a crossover boundary take a free unit and a work-list entry, the others name the
// parental unit) + the stitch's work-list length and the segment totals of the status block: k_pool_publish follows on the same
// stream, which is joined before the stitch starts and the status block leaves
static int enqueue_pool_assign(gev_ctx* c, gev_ctx::Scratch& sc, size_t n_people, hipStream_t st)
{
    if (!c->dense || !sc.n_chrwork) return GEV_OK;
    const size_t rows = 2 * n_people, T = n_people * (size_t)c->nchr;
    SampleDev sd = make_sd(c, sc, T);
    u32 lg = 0; while ((1u << lg) * POOL_INH < sc.nseg_max) lg++;    // threads per row of k_pool_inherit: 2^lg, rows per block: 256 >> lg
    hipLaunchKernelGGL(k_pool_inherit, dim3((unsigned)ceil_div(rows, (size_t)(256u >> lg)), sc.n_chrwork), dim3(256), 0, st, sc.chrwork, rows, c->nchr, sd, lg);
    hipLaunchKernelGGL(k_pool_fresh, dim3((unsigned)ceil_div(rows, 256), sc.n_chrwork), dim3(256), 0, st, sc.chrwork, rows, c->nchr, sd);
    KCHECK();
    return enqueue_pool_publish(c, sc, n_people, st);
}
// sparse state: mutation lists + ancestry intervals (count -> segmented scan -> fill).  Needs the sampling results and the couples;
// nothing of the generation's dense / CV / A-D work reads its output.
static int enqueue_lists(gev_ctx* c, gev_ctx::Scratch& sc, size_t n_people, bool has_mut, hipStream_t st)
{
    const unsigned na = sc.n_chrwork;
    if (!na) return GEV_OK;
    const int nchr = c->nchr;
    const size_t T = n_people * (size_t)nchr, rows = 2 * n_people;
    SampleDev sd = make_sd(c, sc, T);
    // one launch: every (offspring row, position range) either names the parent's pieces or builds its own (gev_lists.h)
    HIPC(hipMemsetAsync(c->d_lp_nitems.p, 0, c->d_lp_nitems.bytes(), st));
    hipLaunchKernelGGL(k_lp_inherit, dim3((unsigned)ceil_div(rows, 256), na), dim3(256), 0, st, sc.chrwork, rows, nchr, (int)has_mut, sd);
    const bool literal = getenv("GEV_LP_LITERAL") && atoi(getenv("GEV_LP_LITERAL")) != 0;      // recombine's statements one by one instead of their closed form (cross-check)
    const dim3 bgrid((unsigned)std::min<size_t>(ceil_div(rows * 4, 256), 2048), na);
    // the planning kernel (a thread plans a piece, the workgroup copies) at every age: over 700 generations at config 2 it stays in
    // front of the eight-lane kernel (host step of the last twenty generations: 0.99 ms against 1.05 ms, of the first twenty: 0.62
    // against 0.72; profiles/r12_age_700_bench.jsonl), so nothing switches by piece length any more.  GEV_LP_LANES=8 selects the eight-lane kernel (tests, comparisons).
    const int lanes = getenv("GEV_LP_LANES") && atoi(getenv("GEV_LP_LANES")) == 8 ? 8 : 1;
    if (literal) hipLaunchKernelGGL((k_lp_build<true>), bgrid, dim3(256), 0, st, sc.chrwork, nchr, (int)has_mut, sd);
    else if (lanes == 1) hipLaunchKernelGGL(k_lp_build_plan, bgrid, dim3(256), 0, st, sc.chrwork, nchr, (int)has_mut, sd);
    else hipLaunchKernelGGL(k_lp_build8, dim3((unsigned)std::min<size_t>(ceil_div(rows * 4, 32), 8192), na), dim3(256), 0, st, sc.chrwork, nchr, (int)has_mut, sd);
    KCHECK();
    return GEV_OK;
}
// CV planes of the offspring: every sub-row (resolved alleles, root-population bits) is inherited by the gamete's crossover
// pattern; the generation's new mutations that fall on a CV position flip the allele there (k_cv_newmut)
// sum_counts (with count_cols, when k_ad_accumulate_wide follows): one launch applies the new mutations and adds k_stitch_small's
// partial counts up, so that the A/D kernel finds the column counts complete (k_cv_newmut_sum)
static int enqueue_cv_planes(gev_ctx* c, gev_ctx::Scratch& sc, size_t n_people, bool has_mut, bool count_cols, bool sum_counts, hipStream_t st)
{
    if (!sc.n_cvwork || !sc.cv_used_max) return GEV_OK;
    const int nchr = c->nchr;
    const size_t T = n_people * (size_t)nchr, rows = 2 * n_people;
    SampleDev sd = make_sd(c, sc, T);
    const CvWork* Vt = sc.cvwork;
    const dim3 grid((unsigned)ceil_div(rows, SMALL_ROWS_PER_BLOCK), sc.n_cvwork); const size_t lds = (size_t)sc.cv_max * sizeof(u64); const u32 nsub = 1u + c->rp_bits;
    // two forms of one launch contract: eight lanes per row where every plane of the launch has the shape for it, else a half-wave per row
    const bool lanes8 = sc.cv_lanes8 && c->cv_stitch_form != 1;
    if (lanes8) hipLaunchKernelGGL(k_stitch_small8, grid, dim3(SMALL8_THREADS), lds, st, Vt, nsub, rows, nchr, sd, sc.cv_max, (int)count_cols);
    else hipLaunchKernelGGL((k_stitch_small<512>), grid, dim3(512), lds, st, Vt, nsub, rows, nchr, sd, sc.cv_max, (int)count_cols);
    c->cv_stitch_launches[lanes8 ? 1 : 0]++;
    if (count_cols && sum_counts) {
        GEVC(c->d_flag.ensure(16, st));                              // (the launch resets the NaN flag of the A/D kernel behind it)
        const unsigned nblk = (unsigned)grid.x, slices = std::min((nblk + 7u) / 8u, 128u);      // eight partial blocks per thread, as k_cv_finish
        const unsigned mut_blocks = has_mut ? (unsigned)ceil_div(n_people, 256) : 0u, col_blocks = (unsigned)std::max<size_t>(ceil_div(sc.cv_max, 256), 1);
        hipLaunchKernelGGL(k_cv_newmut_sum, dim3(mut_blocks + col_blocks * slices, sc.n_cvwork), dim3(256), 0, st, Vt, sc.chrwork, n_people, nchr, sd,
                           mut_blocks, col_blocks, slices, nblk, c->d_flag.as<u32>());
    } else if (has_mut) hipLaunchKernelGGL(k_cv_newmut, dim3((unsigned)ceil_div(n_people, 256), sc.n_cvwork), dim3(256), 0, st, Vt, sc.chrwork, n_people, nchr, sd, (int)count_cols);
    KCHECK();
    return GEV_OK;
}
// the HBM-bound part, on stream_big, after the small work of the same generation: ONE launch over (parent, chromosome)
static int enqueue_stitch(gev_ctx* c, gev_ctx::Scratch& sc, int pop, size_t n_people)
{
    const int nchr = c->nchr;
    const size_t T = n_people * (size_t)nchr, rows = 2 * n_people;
    hipStream_t sb = c->stream_big;
    SampleDev sd = make_sd(c, sc, T);
    HIPC(hipStreamWaitEvent(sb, sc.ev[EV_SMALL_DONE], 0));        // recorded once the unit-table and list streams are joined: unit table, work list, sampling results and couples are complete
    HIPC(hipEventRecord(sc.t[4], sb));
    if (c->dense && sc.n_chrwork) {
        if (rows > 0x7fffffffull) return fail(GEV_EINVAL, "reproduce: stitch grid too large");
        if (c->stitch_mode == 0) {
            // persistent grid over the work list (its length is known to the device only): enough workgroups to fill every CU
            // one wave per entry when the list is as long as the last one; the kernel loops if it is longer
            size_t est = 0;
            for (int k = 0; k < nchr; k++) if (c->chr_active[k]) est = std::max<size_t>(est, c->pop[pop].st[k].pool_last_taken);
            if (!c->alias_rows || !est) est = rows * c->pop[pop].cs[0].nseg;
            // (at most 16384 workgroups of 4 waves = 4 work-list entries each per chromosome; one 16-byte chunk per lane in flight:
            // a 2 KiB segment is one step of a wave -- with 8 KiB segments 2 chunks gave 722, 4 gave 778 generations/s)
            const unsigned nblk = (unsigned)std::min<size_t>(std::max<size_t>(ceil_div(est + est / 8, 4), 256), 16384);
            hipLaunchKernelGGL((k_stitch_segments<true, 1>), dim3(nblk, sc.n_chrwork), dim3(256), 0, sb, sc.chrwork, nchr, sd);
        } else
            hipLaunchKernelGGL(k_stitch_rows, dim3((unsigned)rows, sc.n_chrwork), dim3(STITCH_THREADS), 0, sb, sc.chrwork, nchr, sd);
        KCHECK();
    }
    HIPC(hipEventRecord(sc.t[3], sb));
    HIPC(hipEventRecord(sc.ev[EV_STITCH_DONE], sb));
    HIPC(hipEventRecord(c->ev_planes, sb));
    sc.timing_pending = true; sc.stitch_pending = true; c->planes_pending = true;
    if (c->serialize) {                                  // no overlap: timings are final right away
        HIPC(hipStreamSynchronize(sb)); GEVC(harvest_timing(c, sc)); sc.stitch_pending = false;
        if (g_graveyard.bytes) g_graveyard.drain(c->device, false);
    }
    return GEV_OK;
}

// ---- Simulation::ras_glob_seed / Simulation::random_mate on the device (gev_mate.h) --------------------------------------------
// n ras_glob_seed() values into vals[0..n) and the engine state behind them into *state_out; the engine state in front comes from
// the host (state_val) or from a device word (state_ptr).  blk holds the rejection counts: its user orders it against every other
// draw into it (a scratch set's own, gev_glob_seeds' own)
static int enqueue_glob(Dev<u32>& blk, hipStream_t st, u32 state_val, const u32* state_ptr, size_t n, u32* vals, u32* state_out, u32* flags)
{
    const u64 n_cand = (u64)n + n / 512 + 512;                  // expected rejections: n / 4444 (2147483646 - 2147000000 of 2147483646 outputs)
    const unsigned nb = (unsigned)ceil_div((size_t)n_cand, REJ_CHUNK);
    GEVC(blk.ensure(nb, st));
    hipLaunchKernelGGL(k_glob_count, dim3(nb), dim3(256), 0, st, state_val, state_ptr, n_cand, blk);
    hipLaunchKernelGGL(k_glob_emit, dim3(nb), dim3(256), 0, st, state_val, state_ptr, (u64)n, n_cand, blk, vals, state_out, flags);
    KCHECK();
    return GEV_OK;
}
// Simulation::random_mate of population P's current generation: pop_size couples into father / mother (physical parent rows, what
// the kernels of gev_reproduce read) and, when d_couples is given, as Couples_Info records; meta[0..1] = num_males_mate,
// num_females_mate; the seed (:2092) comes from the host (seed_val) or from a device word (seed_ptr)
static int enqueue_mate(gev_ctx* c, hipStream_t st, PopState& P, u32 seed_val, const u32* seed_ptr, const double* d_svf, size_t pop_size,
                        u32* father, u32* mother, gev_couple* d_couples, u32* meta, u32* flags)
{
    const size_t n_h = P.n_people;
    const u32* logical = nullptr;
    if (!P.logical.empty()) {                                   // after a cross-GPU migration positions are not rows
        GEVC(upload_table(c, c->d_logical, P.logical.data(), n_h, st));
        logical = c->d_logical;
    }
    const unsigned nb = (unsigned)ceil_div(n_h, MATE_CHUNK);
    GEVC(c->mate.flag.ensure(n_h, st)); GEVC(c->mate.blk.ensure(nb, st));
    GEVC(c->mate.posm.ensure(n_h, st)); GEVC(c->mate.posf.ensure(n_h, st));
    hipLaunchKernelGGL(k_mate_flags, dim3(nb), dim3(256), 0, st, P.d_sex[P.cur], logical, d_svf, n_h, seed_val, seed_ptr, c->mate.flag, c->mate.blk);
    hipLaunchKernelGGL(k_mate_compact, dim3(nb), dim3(256), 0, st, c->mate.flag, n_h, c->mate.blk, nb, c->mate.posm, c->mate.posf, meta, flags);
    // candidates of the two pick streams: a draw is rejected with probability < n_h / 2^31
    const u64 n_cand = (u64)pop_size + (u64)(2.0 * (double)pop_size * (double)n_h / 2147483648.0) + 1024;
    const unsigned nbp = (unsigned)ceil_div((size_t)n_cand, REJ_CHUNK);
    GEVC(c->mate.pickblk.ensure(2 * (size_t)nbp, st));
    hipLaunchKernelGGL(k_pick_count, dim3(nbp, 2), dim3(256), 0, st, seed_val, seed_ptr, (const u32*)meta, n_cand, c->mate.pickblk);
    hipLaunchKernelGGL(k_pick_emit, dim3(nbp, 2), dim3(256), 0, st, seed_val, seed_ptr, (const u32*)meta, (u64)pop_size, n_cand, c->mate.pickblk,
                       c->mate.posm, c->mate.posf, logical, father, mother, d_couples, flags);
    KCHECK();
    return GEV_OK;
}

// Hand-overs between the streams of an attempt: `ev` is recorded on `from`, and `to` waits for it -- at once (hand_over) or at a later
// point (hand_record, hand_wait).  Nothing to do where both are the same stream (serialised mode: stream order does it)
static int hand_record(hipStream_t from, hipStream_t to, hipEvent_t ev) { if (from != to) HIPC(hipEventRecord(ev, from)); return GEV_OK; }
static int hand_wait(hipStream_t from, hipStream_t to, hipEvent_t ev) { if (from != to) HIPC(hipStreamWaitEvent(to, ev, 0)); return GEV_OK; }
static int hand_over(hipStream_t from, hipStream_t to, hipEvent_t ev) { GEVC(hand_record(from, to, ev)); return hand_wait(from, to, ev); }
// One attempt of a generation: sampling (unless the head start covers it), lists + CV planes + unit table, the dense stitch on its
// own stream, A/D, and the status block on its way back -- everything enqueued, nothing waited for.  A generation begun with
// gev_generation_begin also draws its ras_glob_seed() values and forms its couples here, on the device.
static int enqueue_attempt(gev_ctx* c, int attempt)
{
    gev_ctx::PendingRepro& q = c->pend;
    gev_ctx::Scratch& sc = c->sc[c->gen_counter & 1];
    PopState& P = c->pop[q.pop];
    // Streams of one attempt.  S carries the chain the host waits for: seeds, sampling, CV planes, A/D, results.
    // X runs what needs neither the sampling nor (for the free list) the couples next to the sampling: Simulation::random_mate and
    // the free list of the segment pool; once the sampling records are complete it builds the unit table and the stitch's work list
    // (k_pool_inherit, k_pool_fresh, k_pool_publish), which only the dense stitch and the status block read, next to the CV planes
    // and A/D.  L builds the mutation / interval lists, which nothing else of the generation reads, there too.  The dense stitch has
    // its own stream as before.  X and L are joined into S before EV_SMALL_DONE and the status block.  Serialised mode (kernel
    // timings without interference): everything on S, in the order CV planes, A/D, unit table, lists.
    hipStream_t S = c->stream, X = c->serialize ? S : c->stream_aux, L = c->serialize ? S : c->stream_list;
    const size_t T = q.n_people * (size_t)c->nchr;
    q.th0 = host_ms();
    if (g_trace_host) HIPC(hipEventRecord(sc.tc[0], S));
    if (attempt == 0) GEVC(harvest_timing(c, sc));          // kernel times of the set's previous generation, before its events are recorded again
    u32* gv = sc.globvals; u32* status = sc.status;
    const bool sampled = q.pre && attempt == 0;              // seeds drawn and sampling done by a head start
    if (q.fused && !sampled) {
        HIPC(hipMemsetAsync(sc.status.p, 0, q.n_status * sizeof(u32), S));
        // glob_generator's draws in the reference's order: random_mate (:2092), reproduce (:2398), then one per (offspring, chromosome) inside ras_add_mutation (:2500).
        // An assortative generation's mating seeds were drawn in front of glob_state: gv[0] = its srand seed (:2170), the rest from glob_state on.
        if (q.assort) {
            HIPC(hipMemsetD32Async((hipDeviceptr_t)gv, (int)q.assort_seed0, 1, S));
            GEVC(enqueue_glob(sc.globblk, S, q.glob_state, nullptr, 1 + (q.has_mut ? T : 0), gv + 1, status + ST_GLOB_STATE, status + ST_FLAGS));
        } else GEVC(enqueue_glob(sc.globblk, S, q.glob_state, nullptr, 2 + (q.has_mut ? T : 0), gv, status + ST_GLOB_STATE, status + ST_FLAGS));
    }
    // (the mating stream starts here: it needs the seeds, not the state behind them)
    GEVC(hand_over(S, X, sc.ev[EV_FORK]));
    if (q.fused && !q.assort) {
        GEVC(enqueue_mate(c, X, P, 0u, gv, q.has_svf ? q.d_svf : nullptr, q.n_people, sc.father, sc.mother,
                          c->d_couples, status + ST_NM_MATE, status + ST_FLAGS));
    }
    if (q.fused && !q.assort && c->chain_draws >= 0) {       // where glob_generator will stand when the host comes back for the next generation
        hipLaunchKernelGGL(k_glob_skip, dim3(1), dim3(64), 0, S, (const u32*)(status + ST_GLOB_STATE), (u32)c->chain_draws, status + ST_NEXT_STATE);
        KCHECK();
        HIPC(hipEventRecord(sc.ev[EV_CHAIN], S));
    }
    GEVC(enqueue_tables(c, sc, q.pop, q.n_people, S));        // (uploaded on S while X mates)
    GEVC(hand_over(S, X, sc.ev[EV_TAB]));
    GEVC(enqueue_pool_free(c, sc, q.pop, X));
    GEVC(hand_record(X, S, sc.ev[EV_AUX]));
    if (q.fused && !sampled) GEVC(enqueue_sampling(c, sc, q.pop, q.n_people, q.has_mut, 0u, S, gv + 1, gv + 2, /*clear_status=*/false));
    else if (!q.fused && !sampled) GEVC(enqueue_sampling(c, sc, q.pop, q.n_people, q.has_mut, q.seed, S));
    // (a head start's records were complete before EV_FORK, which X has waited for; records sampled here are complete behind EV_RECS)
    if (!sampled) GEVC(hand_record(S, X, sc.ev[EV_RECS]));
    q.th1 = host_ms();
    GEVC(hand_wait(X, S, sc.ev[EV_AUX]));
    HIPC(hipEventRecord(sc.t[5], S));
    GEVC(hand_record(S, L, sc.ev[EV_FORKED]));                  // couples and sampling records are complete: what the lists need
    // The unit table, the stitch's work list and their counters: behind the free list in X's own order, next to the CV planes and
    // A/D (nothing on S reads or writes what the pool kernels write).  A repeated attempt's rebuild of the free list is in front of
    // them by the same stream order.  The host enqueues slower than the device runs the first kernels of a generation: the table
    // goes in front of S's CV planes and A/D, because X is idle once it has mated and S waits for the table in the end (both orders
    // measured: DESIGN.md, section 10); the list kernels, which nothing of the generation reads, go last.
    if (!sampled) GEVC(hand_wait(S, X, sc.ev[EV_RECS]));
    if (X != S) GEVC(enqueue_pool_assign(c, sc, q.n_people, X));   // (the one difference of serialised mode: there it goes behind A/D, below)
    GEVC(hand_record(X, S, sc.ev[EV_POOL]));
    // the column counters are filled while the planes are written only if the A/D kernels that consume (and clear) them follow in this attempt
    const bool ad_now = c->eager_ad && c->multipop_ready;
    const bool count_cols = ad_now && sc.cv_count_fused && sc.n_cvwork && sc.cv_used_max;
    // ... and where k_ad_accumulate_wide follows, the launch behind the planes adds the counts up and that kernel computes its terms
    // from them: two launches from the planes to A/D.  The A/D kernel's last block leaves the counters zero, whatever this attempt's
    // records held, so a repeated attempt starts as a first one does.
    const bool sum_counts = count_cols && choose_ad_path(c, q.pop, nullptr, nullptr) == AD_PATH_WIDE;
    GEVC(enqueue_cv_planes(c, sc, q.n_people, q.has_mut, count_cols, sum_counts, S));
    HIPC(hipEventRecord(sc.t[2], S));
    q.th2 = host_ms();
    if (c->ad_cached_pop != q.pop) c->ad_cached_pop = -1;    // (the device-side arrays are about to be rewritten; the published values of q.pop stay readable in their pinned buffer)
    c->ad_host_set_pop = -1;
    if (ad_now) GEVC(enqueue_ad(c, q.pop, c->pop[q.pop].cur ^ 1, q.n_people, sum_counts ? AD_COUNTS_DONE : count_cols ? AD_COUNTS_PARTIAL : AD_COUNTS_NONE, (int)(c->gen_counter & 1)));   // Simulation::ras_compute_AD always follows (src/Simulation.cpp:1935)
    if (g_trace_host) HIPC(hipEventRecord(sc.tc[1], S));
    if (X == S) GEVC(enqueue_pool_assign(c, sc, q.n_people, S));   // serialised: behind A/D, in front of the lists
    GEVC(hand_wait(S, L, sc.ev[EV_FORKED]));
    // Human::sex of the new generation (:2472) for the next gev_random_mate; a fused generation also sends them to the host with the status block
    HIPC(hipMemcpyAsync(P.d_sex[P.cur ^ 1].p, sc.sex.p, q.n_people, hipMemcpyDeviceToDevice, L));
    if (P.ids_ok) {                                          // the offspring's pedigree ids (:2473-2479) from the parents' rows, into the other buffer
        const int nb = P.ibuf ^ 1;
        GEVC(P.d_ids[nb].ensure(PED_FIELDS * q.n_people, L)); GEVC(P.d_cidx[nb].ensure(q.n_people, L));
        P.ids_stride[nb] = q.n_people;
        hipLaunchKernelGGL(k_ped_offspring, dim3((unsigned)ceil_div(q.n_people, 256)), dim3(256), 0, L, P.d_ids[P.ibuf], P.ids_stride[P.ibuf],
                           P.n_phys, sc.father, sc.mother, q.n_people, P.d_ids[nb], q.n_people,
                           q.cidx_mode == 1 ? sc.cidx : (const u32*)nullptr, q.cidx_mode == 2 ? c->am.ooff : (const u32*)nullptr,
                           (u32)q.n_couples, P.d_cidx[nb]);
        KCHECK();
    }
    if (q.fused) { HIPC(hipMemcpyAsync(q.hsex, sc.sex.p, q.n_people, hipMemcpyDeviceToHost, L)); HIPC(hipMemcpyAsync(q.hseeds2, gv, 2 * sizeof(u32), hipMemcpyDeviceToHost, L)); }   // (copies nothing on the device waits for: off the main stream)
    GEVC(enqueue_lists(c, sc, q.n_people, q.has_mut, L));
    GEVC(hand_over(L, S, sc.ev[EV_LISTS]));
    GEVC(hand_wait(X, S, sc.ev[EV_POOL]));                        // unit table, work list and the status block's segment totals
    if (g_trace_host) HIPC(hipEventRecord(sc.tc[2], S));
    // The dense stitch needs the sampling results, the couples and the unit table only, but it saturates HBM, and every
    // latency-bound kernel that runs next to it takes 2-5 times as long (and slows it down in turn).  Behind the whole small work,
    // at the small kernels' priority, it runs alone for 0.16 ms next to the host's turn-around; the NEXT generation's ALU-bound
    // sampling (head start) is what shares the GPU with it (streams).
    HIPC(hipEventRecord(sc.ev[EV_SMALL_DONE], S)); GEVC(enqueue_stitch(c, sc, q.pop, q.n_people));
    HIPC(hipMemcpyAsync(q.hstatus, sc.status.p, q.n_status * sizeof(u32), hipMemcpyDeviceToHost, S));
    HIPC(hipEventRecord(sc.ev_status, S));                  // gev_reproduce_end waits for THIS, not for whatever a head start queued behind it
    sc.th_enq = host_ms();
    return GEV_OK;
}
// The size checks every call that samples a generation makes (who: the prefix of its messages)
static int check_sizes(gev_ctx* c, const char* who, size_t n_people, const uint32_t* mut_seeds, size_t n_mut_seeds)
{
    const size_t T = n_people * (size_t)c->nchr;
    if (n_people == 0) return fail(GEV_EINVAL, "%s: no offspring", who);
    if (2 * T * GEV_BK_CAP >= 0xf0000000ull) return fail(GEV_EINVAL, "%s: too many gametes", who);
    if (mut_seeds && n_mut_seeds != T) return fail(GEV_EINVAL, "%s: n_mut_seeds=%zu, expected n_people*nchr=%zu", who, n_mut_seeds, T);
    return GEV_OK;
}
// What the begin calls share: the size checks, the static tables, room for n_people offspring, the pinned staging buffer
// [status | extra_bytes of the caller's] and the fields of the pending generation (c->pend) that do not depend on who begins it;
// the caller sets what is its own.  fused: the library draws the mutation seeds itself wherever the population has a mutation map
// (and the extra bytes start with the two seeds and the sexes that go back to the host); otherwise the caller's mut_seeds say
static int begin_prologue(gev_ctx* c, int pop, const char* who, size_t n_people, bool fused, const uint32_t* mut_seeds, size_t n_mut_seeds, size_t extra_bytes)
{
    GEVC(check_sizes(c, who, n_people, mut_seeds, n_mut_seeds));
    bool has_mut = mut_seeds != nullptr;
    if (fused) GEVC(population_has_mutmap(c, pop, has_mut));
    if (!has_mut) GEVC(check_chain_size(n_people * (size_t)c->nchr));
    const size_t n_status = ST_TOTALS + ST_PER_CHR * (size_t)c->nchr;
    const size_t stage_bytes = n_status * sizeof(u32) + extra_bytes;
    GEVC(c->h_stage.ensure(stage_bytes, stage_bytes * 5 / 4 + 4096, nullptr));
    GEVC(finalize_static(c, pop));
    GEVC(prepare_eager_ad(c, pop));
    GEVC(ensure_capacity(c, pop, n_people));
    gev_ctx::PendingRepro& q = c->pend;
    q.pop = pop; q.n_people = n_people; q.has_mut = has_mut; q.pre = false; q.seed = 0; q.attempt = 0; q.n_status = n_status; q.hstatus = (u32*)c->h_stage.p;
    q.pool_rebuilt = false;
    q.fused = fused; q.has_svf = false; q.d_svf = nullptr; q.hseeds2 = q.hstatus + n_status; q.hsex = (uint8_t*)(q.hseeds2 + 2);
    q.assort = false; q.cidx_mode = 0; q.n_couples = n_people;
    return GEV_OK;
}
// gev_reproduce in two halves: _begin checks and stages the inputs and enqueues the generation's device work, _end waits for it,
// repeats it with larger buffers if a capacity was exceeded, and publishes the new generation.  Between the two the host is free
// (the bench forms the next generation's couples there); no other call on the context is allowed in between.
int gev_reproduce_begin(gev_ctx* c, int pop, const gev_couple* couples, size_t n_couples, uint32_t seed_reproduce,
                        const uint32_t* mut_seeds, size_t n_mut_seeds, size_t n_people)
{
    GEVC(check_idx(c, pop, 0));
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "reproduce: population %d has no current generation (call gev_init_gen0)", pop);
    HIPC(hipSetDevice(c->device));
    const size_t T = n_people * (size_t)c->nchr;
    const bool has_mut = mut_seeds != nullptr;
    // pinned staging behind the status block: [father | mother | mut_seeds | cidx], written by the host, copied asynchronously
    // (the prologue fills c->pend and runs finalize_static / ensure_capacity although the call may still be refused below: nothing
    // reads c->pend while pend.active is false, which only the end of this function sets)
    GEVC(begin_prologue(c, pop, "reproduce", n_people, /*fused=*/false, mut_seeds, n_mut_seeds, (2 * n_people + (has_mut ? T : 0) + (c->track_pedigree ? n_people : 0)) * sizeof(u32)));
    gev_ctx::PendingRepro& q = c->pend;
    gev_ctx::Scratch& sc = c->sc[c->gen_counter & 1];
    // couples == NULL: the couples gev_random_mate left on the device for this population
    const bool dev_couples = couples == nullptr;
    if (dev_couples && !(sc.mated && sc.mate_pop == pop && sc.mate_n == n_people))
        return fail(GEV_ESTATE, "reproduce: couples is NULL but no gev_random_mate / gev_assort_mate of population %d for %zu offspring precedes", pop, n_people);
    if (dev_couples && sc.mate_epoch != P.layout_epoch)
        return fail(GEV_ESTATE, "reproduce: couples is NULL but population %d changed (migration, rows removed or imported, order materialised) "
                    "after the gev_random_mate / gev_assort_mate that formed them: its positions no longer name the same rows", pop);
    u32* father = q.hstatus + q.n_status; u32* mother = father + n_people; u32* hseeds = mother + n_people;
    u32* hcidx = hseeds + (has_mut ? T : 0);                 // (tracking only) index of every child's couple in `couples`
    // offspring enumeration order of the couple loop (src/Simulation.cpp:2433-2443)
    size_t ip = 0;
    const u32* lg = P.logical.empty() ? nullptr : P.logical.data();
    for (size_t it = 0; it < n_couples && !dev_couples; it++) {
        if (couples[it].inbreed) continue;
        if (couples[it].num_offspring < 0) return fail(GEV_EINVAL, "reproduce: couple %zu has negative num_offspring", it);
        if (couples[it].num_offspring && (couples[it].pos_male >= P.n_people || couples[it].pos_female >= P.n_people))
            return fail(GEV_EINVAL, "reproduce: couple %zu references position beyond the population (%zu people)", it, P.n_people);
        for (int ns = 0; ns < couples[it].num_offspring; ns++) {
            if (ip >= n_people) return fail(GEV_EINVAL, "reproduce: n_people=%zu but the couples list yields more offspring", n_people);
            father[ip] = lg ? lg[couples[it].pos_male] : (u32)couples[it].pos_male;
            mother[ip] = lg ? lg[couples[it].pos_female] : (u32)couples[it].pos_female;
            if (c->track_pedigree) hcidx[ip] = (u32)it;
            ip++;
        }
    }
    if (!dev_couples && ip != n_people) return fail(GEV_EINVAL, "reproduce: n_people=%zu but the couples list yields %zu offspring", n_people, ip);
    hipStream_t st = c->stream;
    // sampling already enqueued by gev_presample for exactly these inputs?
    GEVC(take_head_start(c, sc, HeadStart::PRESAMPLE, pop, n_people, has_mut, (u32)seed_reproduce, mut_seeds, q.pre));
    if (!q.pre) {
        // the stitch that last read this scratch set must be over before the set is refilled
        GEVC(claim_scratch(c, sc, st, true, n_people, has_mut));
        if (has_mut) { memcpy(hseeds, mut_seeds, T * sizeof(u32)); HIPC(hipMemcpyAsync(sc.mutseeds.p, hseeds, T * sizeof(u32), hipMemcpyHostToDevice, st)); }
    }
    if (!dev_couples) {
        HIPC(hipMemcpyAsync(sc.father.p, father, n_people * sizeof(u32), hipMemcpyHostToDevice, st));
        HIPC(hipMemcpyAsync(sc.mother.p, mother, n_people * sizeof(u32), hipMemcpyHostToDevice, st));
        if (P.ids_ok) { GEVC(sc.cidx.ensure(n_people, st)); HIPC(hipMemcpyAsync(sc.cidx.p, hcidx, n_people * sizeof(u32), hipMemcpyHostToDevice, st)); }
    }
    q.seed = (u32)seed_reproduce;
    if (!dev_couples) { q.cidx_mode = 1; q.n_couples = n_couples; }
    else if (sc.mate_assort) { q.cidx_mode = 2; q.n_couples = (size_t)c->am.res.n_couples; }
    GEVC(enqueue_attempt(c, 0));
    q.active = true;
    return GEV_OK;
}
static int enqueue_chain_head_start(gev_ctx* c)
{
    gev_ctx::PendingRepro& q = c->pend;
    gev_ctx::Scratch& sc = c->sc[c->gen_counter & 1]; gev_ctx::Scratch& nx = c->sc[(c->gen_counter + 1) & 1];
    hipStream_t SS = c->serialize ? c->stream : c->stream_samp;
    const size_t T = q.n_people * (size_t)c->nchr;
    // the stitch that last read the other scratch set (the previous generation's) may still be running: the sampling stream waits for
    // it, the host does not (its kernel time is collected when the set's next generation is enqueued)
    GEVC(claim_scratch(c, nx, SS, false, q.n_people, q.has_mut));   // (sizes the buffers in front of the wait below: allocations only, no stream work)
    HIPC(hipStreamWaitEvent(SS, sc.ev[EV_CHAIN], 0));
    GEVC(nx.globvals.ensure((2 + T), SS));
    u32* gv = nx.globvals; u32* status = nx.status;
    HIPC(hipMemsetAsync(nx.status.p, 0, q.n_status * sizeof(u32), SS));
    GEVC(enqueue_glob(nx.globblk, SS, 0u, sc.status + ST_NEXT_STATE, 2 + (q.has_mut ? T : 0), gv, status + ST_GLOB_STATE, status + ST_FLAGS));
    GEVC(enqueue_sampling(c, nx, q.pop, q.n_people, q.has_mut, 0u, SS, gv + 1, gv + 2, /*clear_status=*/false));
    HIPC(hipEventRecord(nx.ev[EV_SAMPLED], SS));
    nx.hs.kind = HeadStart::CHAIN; nx.hs.dropped = false; nx.hs.pop = q.pop; nx.hs.n_people = q.n_people; nx.hs.has_mut = q.has_mut;
    return GEV_OK;
}
// A/D is computed with the generation (same enqueue, same wait) once the per-population a/d tables exist; they are set up by the
// first gev_compute_ad, or here as soon as every population of the context has its static inputs
static int prepare_eager_ad(gev_ctx* c, int pop)
{
    if (c->multipop_ready) return GEV_OK;
    for (const PopState& Q : c->pop)
        for (int k = 0; k < c->nchr; k++) {
            if (Q.cs[k].rbp.empty() || (c->chr_active[k] && Q.cs[k].pos.empty() && Q.cs[k].L)) return GEV_OK;
            for (int p = 0; p < c->nphen; p++) if (c->chr_active[k] && !Q.cv[p][k].set) return GEV_OK;
        }
    return check_multipop(c);
}
// does every chromosome of the population have a mutation map (Simulation::reproduce's `_mutation_map.size() > 0`, :2459)?
// Without a mutation map every gamete's seed is a rand() of the srand() of the gamete before it (src/Simulation.cpp:2447-2455):
// the 2 T gametes form one serial chain, a few microseconds each on one workgroup (k_rec_chain_wg).  Beyond GEV_CHAIN_MAX_TASKS
// (default 4 000 000 tasks: tens of seconds per generation) the call refuses instead of running for minutes.
static int check_chain_size(size_t T)
{
    const size_t chain_max = getenv("GEV_CHAIN_MAX_TASKS") ? (size_t)atoll(getenv("GEV_CHAIN_MAX_TASKS")) : (size_t)4000000;
    if (T > chain_max)
        return fail(GEV_EUNSUPPORTED, "Error: %zu (offspring, chromosome) tasks without a mutation map form one serial rand() chain; more than %zu are refused (GEV_CHAIN_MAX_TASKS) -- give a mutation map (rates may be 0) to sample the tasks in parallel", T, chain_max);
    return GEV_OK;
}
static int population_has_mutmap(gev_ctx* c, int pop, bool& has_mut)
{
    PopState& P = c->pop[pop];
    has_mut = P.cs[0].mut_set;
    for (int k = 1; k < c->nchr; k++)
        if (P.cs[k].mut_set != has_mut) return fail(GEV_ESTATE, "population %d: a mutation map is set for some chromosomes only", pop);
    return GEV_OK;
}
// One generation of a randomly mating population in one piece: Simulation::random_mate -> Simulation::reproduce ->
// Simulation::ras_compute_AD (the body of sim_next_generation, src/Simulation.cpp:1907-1935) with every ras_glob_seed() value
// the three draw -- 1 (:2092) + 1 (:2398) + n_people * nchr (:2500) -- taken from glob_generator's state ON THE DEVICE.
// selection_value_func: host array (uploaded) or NULL; dev_sel: the population's own device values (gev_compute_selection) instead
static int generation_begin(gev_ctx* c, int pop, uint32_t glob_state, size_t pop_size, const double* selection_value_func, bool dev_sel)
{
    GEVC(check_idx(c, pop, 0));
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "generation: population %d has no current generation (call gev_init_gen0)", pop);
    if (glob_state == 0 || glob_state >= GEV_M31) return fail(GEV_EINVAL, "generation: %u is not a state of std::minstd_rand0 (1 .. 2^31-2)", glob_state);
    HIPC(hipSetDevice(c->device));
    const size_t n_people = pop_size;
    // pinned: [status | the two seeds | sexes]
    GEVC(begin_prologue(c, pop, "generation", n_people, /*fused=*/true, nullptr, 0, 2 * sizeof(u32) + n_people + 16));
    gev_ctx::PendingRepro& q = c->pend;
    hipStream_t st = c->stream;
    gev_ctx::Scratch& sc = c->sc[c->gen_counter & 1];
    // seeds already drawn and sampling already enqueued for exactly this call (gev_set_generation_chain)?
    GEVC(take_head_start(c, sc, HeadStart::CHAIN, pop, n_people, q.has_mut, (u32)glob_state, nullptr, q.pre));
    if (!q.pre) {
        GEVC(claim_scratch(c, sc, st, true, n_people, q.has_mut));
        GEVC(sc.globvals.ensure((2 + n_people * (size_t)c->nchr), st));
    }
    GEVC(c->d_couples.ensure(n_people, st));
    if (selection_value_func) {
        GEVC(c->mate.svf.ensure(P.n_people, st));
        HIPC(hipMemcpyAsync(c->mate.svf.p, selection_value_func, P.n_people * sizeof(double), hipMemcpyHostToDevice, st));
        HIPC(hipStreamSynchronize(st));                          // the caller's array is pageable memory of unknown lifetime
    }
    const double* d_svf = selection_value_func ? c->mate.svf : nullptr;
    if (dev_sel) d_svf = P.d_sel[P.sbuf] + 2 * P.n_people;     // (enqueued on this stream behind gev_compute_selection: no wait)
    q.has_svf = d_svf != nullptr; q.d_svf = d_svf; q.glob_state = glob_state;
    GEVC(enqueue_attempt(c, 0));
    q.active = true;
    if (c->chain_draws >= 0) GEVC(enqueue_chain_head_start(c));    // behind this generation's work: the next generation waits for all of it
    return GEV_OK;
}
int gev_generation_begin(gev_ctx* c, int pop, uint32_t glob_state, size_t pop_size, const double* selection_value_func)
{
    return generation_begin(c, pop, glob_state, pop_size, selection_value_func, false);
}
static int check_selection(gev_ctx* c, int pop, const char* who)
{
    GEVC(check_idx(c, pop, 0));
    if (c->pend.active) return fail(GEV_ESTATE, "%s: a generation is pending: call gev_generation_end / gev_reproduce_end first", who);
    const PopState& P = c->pop[pop];
    if (!P.gen0 || !P.sel_ok)
        return fail(GEV_ESTATE, "%s: population %d has no selection values of its current generation on the device (gev_compute_selection)", who, pop);
    return GEV_OK;
}
int gev_generation_begin_selected(gev_ctx* c, int pop, uint32_t glob_state, size_t pop_size)
{
    GEVC(check_selection(c, pop, "generation_begin_selected"));
    return generation_begin(c, pop, glob_state, pop_size, nullptr, true);
}
// The host announced how many ras_glob_seed() values it draws itself between two generations (gev_set_generation_chain): the state
// glob_generator will have at the next gev_generation_begin is then known on the device as soon as this generation's seeds are
// drawn.  Draw the NEXT generation's seeds from it and run its sampling now, on the head-start stream, into the other scratch
// set: it shares the GPU with this generation's dense stitch (ALU-bound next to HBM-bound) instead of standing in front of the
// next generation's small work.  The next gev_generation_begin recognises it by the engine state it is handed.
int gev_set_generation_chain(gev_ctx* c, int draws_between)
{
    GEVC(check_not_pending(c));
    if (draws_between > 1000000) return fail(GEV_EINVAL, "set_generation_chain: %d draws between two generations", draws_between);
    c->chain_draws = draws_between < 0 ? -1 : draws_between;
    return GEV_OK;
}
static int generation_finish_inner(gev_ctx* c, uint8_t* sex_out, gev_generation_result* res, gev_couple* couples_out);
static int generation_finish(gev_ctx* c, uint8_t* sex_out, gev_generation_result* res, gev_couple* couples_out)
{
    const int rc = generation_finish_inner(c, sex_out, res, couples_out);
    if (rc != GEV_OK) c->ad_cached_pop = -1;                 // the device-side A/D arrays hold a generation that was not published
    return rc;
}
static int generation_finish_inner(gev_ctx* c, uint8_t* sex_out, gev_generation_result* res, gev_couple* couples_out)
{
    gev_ctx::PendingRepro& q = c->pend;
    q.active = false;                                       // whatever happens below, the generation is no longer pending
    HIPC(hipSetDevice(c->device));
    const int pop = q.pop, nchr = c->nchr; const size_t n_people = q.n_people;
    PopState& P = c->pop[pop];
    hipStream_t st = c->stream;
    gev_ctx::Scratch& sc = c->sc[c->gen_counter & 1];
    u32* hstatus = q.hstatus;
    const int alt = P.cur ^ 1;
    for (int attempt = q.attempt;; attempt++) {
        if (attempt > 0) GEVC(enqueue_attempt(c, attempt));
        const double th_w0 = host_ms();
        HIPC(hipEventSynchronize(sc.ev_status));
        const u32 flags = hstatus[ST_FLAGS];
        if (g_trace_host) {
            static double last_status = 0; const double now = host_ms();
            float a = 0, b = 0, d = 0, e = 0;
            (void)hipEventSynchronize(sc.tc[2]); (void)hipEventElapsedTime(&a, sc.tc[0], sc.t[5]); (void)hipEventElapsedTime(&b, sc.t[5], sc.t[2]); (void)hipEventElapsedTime(&d, sc.t[2], sc.tc[1]); (void)hipEventElapsedTime(&e, sc.tc[1], sc.tc[2]);
            fprintf(stderr, "[gev] gen %u host: since last status %.3f = to first launch %.3f + enqueue %.3f + host idle %.3f + wait %.3f | device chain: to CV planes %.3f, CV planes %.3f, A/D %.3f, unit table + lists after A/D %.3f\n",
                    c->gen_counter, now - last_status, q.th0 - last_status, sc.th_enq - q.th0, th_w0 - sc.th_enq, now - th_w0, a, b, d, e);
            last_status = now;
        }
        if (g_trace_host) fprintf(stderr, "[gev] gen %u attempt %d pre %d: enqueue sampling %.2f ms, sparse %.2f ms, A/D + wait %.2f ms, flags %u, graveyard %.1f MiB\n",
                                  c->gen_counter, attempt, (int)q.pre, q.th1 - q.th0, q.th2 - q.th1, host_ms() - q.th2, flags, g_graveyard.bytes / 1048576.0);
        if (g_trace_host && g_malloc_n) { fprintf(stderr, "[gev]   %zu hipMalloc calls, %.1f MiB, %.2f ms\n", g_malloc_n, g_malloc_bytes / 1048576.0, g_malloc_ms); g_malloc_ms = 0; g_malloc_n = 0; g_malloc_bytes = 0; }
        for (int k = 0; k < nchr; k++) { P.st[k].lp.m_last = hstatus[ST_TOTALS + ST_PER_CHR * k]; P.st[k].lp.p_last = hstatus[ST_TOTALS + ST_PER_CHR * k + 1]; }   // entries appended to the arenas
        if (c->dense) for (int k = 0; k < nchr; k++) if (c->chr_active[k]) {
            ChrState& cs = P.st[k]; const u32* stw = hstatus + ST_TOTALS + ST_PER_CHR * k;
            cs.pool_n_free = stw[4]; cs.pool_cursor = stw[5]; cs.pool_last_taken = stw[2];
        }
        if ((flags & FLAG_POOL) && q.pool_rebuilt) return fail(GEV_EDEVICE, "reproduce: genotype row pool exhausted (internal error)");
        if (flags & FLAG_RNG_SHORT) return fail(GEV_EDEVICE, "generation: a rejection stream ran out of candidates (internal error)");
        if (flags & FLAG_NO_MATES)                          // Simulation::random_mate returns false (:2125-2129); nothing is published
            return fail(GEV_ENOMATE, "Error: No one can marry, num_males_mate=%u, num_females_mate=%u", hstatus[ST_NM_MATE], hstatus[ST_NF_MATE]);
        if (!(flags & (FLAG_REDO_MASK | FLAG_POOL))) break;
        if (flags & FLAG_POOL) { for (int k = 0; k < nchr; k++) P.st[k].pool_force_rebuild = true; q.pool_rebuilt = true; }   // the free list ran out: rebuild it, then the generation again
        if (attempt == 3) return fail(GEV_EDEVICE, "reproduce: buffers still too small after %d attempts (flags %u)", attempt + 1, flags);
        HIPC(hipStreamSynchronize(c->stream_big));        // the stitch of the failed attempt still reads the records that are sampled again below
        sc.timing_pending = false; sc.stitch_pending = false;   // (its kernel times are not counted)
        {   // a head start taken meanwhile used the old record capacities: it is sampled again (by gev_presample_sex from the retained
            // inputs, or by the next gev_reproduce_begin)
            gev_ctx::Scratch& nx = c->sc[(c->gen_counter + 1) & 1];
            drop_head_start(nx);
        }
        if (flags & FLAG_BK_OVF) c->bk_ovf_cap = std::max<size_t>(2 * c->bk_ovf_cap, (size_t)hstatus[ST_BK_OVF_USED] * 5 / 4 + 1024);
        if (flags & FLAG_NM_OVF) c->nm_ovf_cap = std::max<size_t>(2 * c->nm_ovf_cap, (size_t)hstatus[ST_NM_OVF_USED] * 5 / 4 + 1024);
        if (flags & FLAG_PARTS_CAP) for (int k = 0; k < nchr; k++) P.st[k].lp.grow_p = c->chr_active[k] && c->track_intervals;   // an arena was full: doubled before the next attempt
        if (flags & FLAG_MUT_CAP) for (int k = 0; k < nchr; k++) P.st[k].lp.grow_m = c->chr_active[k];
        c->redo_count++; if (flags & FLAG_POOL) c->redo_pool_count++;
    }
    for (int k = 0; k < nchr; k++) if (c->chr_active[k]) {      // the offspring's pieces are the state now; the CSR form is made when somebody asks for it
        ChrState::LpState& lp = P.st[k].lp;
        lp.p_used += lp.p_last; lp.m_used += lp.m_last; P.st[k].csr_valid = false;
    }
    if (c->dense) for (int k = 0; k < nchr; k++) if (c->chr_active[k]) {            // 16-byte chunks the stitch wrote / chunks of the generation's rows
        const ChrStatic& S = P.cs[k];
        const unsigned long long units = hstatus[ST_TOTALS + ST_PER_CHR * k + 2], last = hstatus[ST_TOTALS + ST_PER_CHR * k + 3];
        const unsigned long long chunks = S.stride / 16, seg = 1ull << S.seg_shift, last_chunks = chunks - (S.nseg - 1) * seg;
        c->chunks_written_sum += (units - last) * seg + last * last_chunks; c->chunks_total_sum += 2ull * n_people * chunks;
        c->segments_written_sum += units; c->segments_total_sum += 2ull * n_people * S.nseg;
    }
    const bool ad_done = c->eager_ad && c->multipop_ready;
    for (int p = 0; p < c->nphen; p++) for (int k = 0; k < nchr; k++) P.cv[p][k].frq_valid = ad_done;
    c->ad_cached_pop = ad_done ? pop : -1;
    if (q.fused) {
        c->chain_valid = !q.assort && c->chain_draws >= 0; c->chain_state = hstatus[ST_NEXT_STATE];     // (no head start behind an assortative generation)
        if (sex_out) memcpy(sex_out, q.hsex, n_people);
        if (res) {
            res->glob_state = hstatus[ST_GLOB_STATE]; res->seed_mate = q.hseeds2[0]; res->seed_reproduce = q.hseeds2[1]; res->reserved = 0;
            res->num_males_mate = q.assort ? q.am_nm : hstatus[ST_NM_MATE]; res->num_females_mate = q.assort ? q.am_nf : hstatus[ST_NF_MATE];
        }
        const size_t n_rec = q.assort ? q.am_couples : n_people;
        if (couples_out) { HIPC(hipMemcpyAsync(couples_out, c->d_couples.p, n_rec * sizeof(gev_couple), hipMemcpyDeviceToHost, st)); HIPC(hipStreamSynchronize(st)); }
    } else if (sex_out) { HIPC(hipMemcpyAsync(sex_out, sc.sex.p, n_people, hipMemcpyDeviceToHost, st)); HIPC(hipStreamSynchronize(st)); }
    P.cur = alt; P.pcur = (P.pcur + 1) % 3; P.n_people = n_people; P.n_phys = n_people; P.logical.clear(); P.layout_epoch++; P.drop_selection();
    if (P.ids_ok) {                                         // (every attempt wrote the offspring's ids and couple indices into the other buffers)
        P.ibuf ^= 1;
        P.cs_ok = true; P.cs_seed = q.fused ? q.hseeds2[1] : q.seed; P.cs_ncouples = q.n_couples;
    }
    c->gen_counter++;
    return GEV_OK;
}
int gev_reproduce_end(gev_ctx* c, uint8_t* sex_out)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (!c->pend.active) return fail(GEV_ESTATE, "reproduce_end: no gev_reproduce_begin is pending");
    if (c->pend.fused) return fail(GEV_ESTATE, "reproduce_end: the pending generation was begun with gev_generation_begin: call gev_generation_end");
    return generation_finish(c, sex_out, nullptr, nullptr);
}
int gev_generation_end(gev_ctx* c, gev_generation_result* res, gev_couple* couples_out, uint8_t* sex_out)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (!c->pend.active) return fail(GEV_ESTATE, "generation_end: no gev_generation_begin is pending");
    if (!c->pend.fused) return fail(GEV_ESTATE, "generation_end: the pending generation was begun with gev_reproduce_begin: call gev_reproduce_end");
    return generation_finish(c, sex_out, res, couples_out);
}
int gev_reproduce(gev_ctx* c, int pop, const gev_couple* couples, size_t n_couples, uint32_t seed_reproduce,
                  const uint32_t* mut_seeds, size_t n_mut_seeds, size_t n_people, uint8_t* sex_out)
{
    GEVC(gev_reproduce_begin(c, pop, couples, n_couples, seed_reproduce, mut_seeds, n_mut_seeds, n_people));
    return gev_reproduce_end(c, sex_out);
}
// Simulation::random_mate (src/Simulation.cpp:2090-2157) of the population's current generation on the device.  The couples stay
// on the device for the next gev_reproduce of the population (couples == NULL there) and are copied out when couples_out is given.
static int random_mate(gev_ctx* c, int pop, uint32_t seed, const double* selection_value_func, bool dev_sel, size_t pop_size, gev_couple* couples_out,
                       size_t* num_males_mate, size_t* num_females_mate)
{
    GEVC(check_idx(c, pop, 0));
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "random_mate: population %d has no current generation", pop);
    if (pop_size == 0) return fail(GEV_EINVAL, "random_mate: no couples asked for");
    if (pop_size >= 0x7fffffffull) return fail(GEV_EINVAL, "random_mate: too many couples");
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    gev_ctx::Scratch& sc = c->sc[c->gen_counter & 1];
    // father / mother of this scratch set were last read by the stitch two generations back
    GEVC(claim_scratch(c, sc, st, true, 0, false));
    GEVC(sc.father.ensure(pop_size, st)); GEVC(sc.mother.ensure(pop_size, st));
    GEVC(c->d_couples.ensure(pop_size, st));
    GEVC(c->mate.stat.ensure(4, st));
    HIPC(hipMemsetAsync(c->mate.stat.p, 0, 4 * sizeof(u32), st));
    const double* d_svf = nullptr;
    if (selection_value_func) {
        GEVC(c->mate.svf.ensure(P.n_people, st));
        HIPC(hipMemcpyAsync(c->mate.svf.p, selection_value_func, P.n_people * sizeof(double), hipMemcpyHostToDevice, st));
        d_svf = c->mate.svf;
    }
    if (dev_sel) d_svf = P.d_sel[P.sbuf] + 2 * P.n_people;
    u32* ms = c->mate.stat;                             // {num_males_mate, num_females_mate, flags}
    GEVC(enqueue_mate(c, st, P, (u32)seed, nullptr, d_svf, pop_size, sc.father, sc.mother, couples_out ? c->d_couples : nullptr, ms, ms + 2));
    u32 h[4] = {0, 0, 0, 0};
    HIPC(hipMemcpyAsync(h, ms, sizeof h, hipMemcpyDeviceToHost, st));
    if (couples_out) HIPC(hipMemcpyAsync(couples_out, c->d_couples.p, pop_size * sizeof(gev_couple), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (num_males_mate) *num_males_mate = h[0];
    if (num_females_mate) *num_females_mate = h[1];
    sc.mated = false;
    if (h[2] & FLAG_NO_MATES) return fail(GEV_ENOMATE, "Error: No one can marry, num_males_mate=%u, num_females_mate=%u", h[0], h[1]);
    if (h[2] & FLAG_RNG_SHORT) return fail(GEV_EDEVICE, "random_mate: a rejection stream ran out of candidates (internal error)");
    sc.mated = true; sc.mate_assort = false; sc.mate_pop = pop; sc.mate_n = pop_size; sc.mate_epoch = P.layout_epoch;
    return GEV_OK;
}
int gev_random_mate(gev_ctx* c, int pop, uint32_t seed, const double* selection_value_func, size_t pop_size, gev_couple* couples_out,
                    size_t* num_males_mate, size_t* num_females_mate)
{
    return random_mate(c, pop, seed, selection_value_func, false, pop_size, couples_out, num_males_mate, num_females_mate);
}
int gev_random_mate_selected(gev_ctx* c, int pop, uint32_t seed, size_t pop_size, gev_couple* couples_out, size_t* num_males_mate, size_t* num_females_mate)
{
    GEVC(check_selection(c, pop, "random_mate_selected"));
    return random_mate(c, pop, seed, nullptr, true, pop_size, couples_out, num_males_mate, num_females_mate);
}
// ---- Simulation::assort_mate (src/Simulation.cpp:2167-2360) on the device (gev_assort.h) -----------------------------------------
size_t gev_sort_pairs_scratch_bytes(size_t n);
int gev_sort_pairs_f64(const double* d_x, const uint32_t* d_gather, const uint32_t* d_vals, size_t n, uint32_t* d_vals_out, void* d_tmp, hipStream_t st);
static int am_sort(gev_ctx* c, hipStream_t st, const double* x, const u32* gather, const u32* vals, size_t n, u32* out)
{
    GEVC(c->am.sort_tmp.ensure(gev_sort_pairs_scratch_bytes(n), st));
    const int e = gev_sort_pairs_f64(x, gather, vals, n, out, c->am.sort_tmp.p, st);
    if (e) return fail(GEV_EDEVICE, "assort_mate: device sort failed: %s", hipGetErrorString((hipError_t)e));
    return GEV_OK;
}
// CommFunc::ras_rank on the device (the O(n^2) host loop of assort_mate, src/Simulation.cpp:2278-2279): stable radix sort of
// order-preserving keys with the reference's tie / NaN rule (gev_sort.hip)
extern "C" size_t gev_rank_scratch_bytes(size_t n);
extern "C" int gev_rank_device(const double* d_x, size_t n, unsigned long long* d_rank, void* d_tmp, hipStream_t st);
int gev_rank_f64(gev_ctx* c, const double* x, size_t n, unsigned long long* rank_out)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (n && (!x || !rank_out)) return fail(GEV_EINVAL, "rank_f64: null buffer");
    if (!n) return GEV_OK;
    if (n >= 0xffffffffull) return fail(GEV_EINVAL, "rank_f64: too many values");
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    GEVC(c->d_tmp.ensure(n * 16, st));
    double* dx = c->d_tmp.as<double>(); unsigned long long* dr = (unsigned long long*)(dx + n);
    HIPC(hipMemcpyAsync(dx, x, n * sizeof(double), hipMemcpyHostToDevice, st));
    GEVC(c->d_text.ensure(gev_rank_scratch_bytes(n), st));
    const int e = gev_rank_device(dx, n, dr, c->d_text.p, st);
    if (e) return fail(GEV_EDEVICE, "rank_f64: HIP error %s in the sort", hipGetErrorString((hipError_t)e));
    HIPC(hipMemcpyAsync(rank_out, dr, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
// std::random_shuffle of m entries on the rand() values R[0 .. m-2]: src[q] = original position of the entry that ends at p0 + q
static int am_shuffle(gev_ctx* c, hipStream_t st, const u32* R, size_t m, size_t p0, size_t p1, Dev<u32>& src)
{
    gev_ctx::AssortState& A = c->am;
    const size_t w = (m + 1) * sizeof(u32);
    GEVC(A.scnt.ensure(m + 1, st)); GEVC(A.soff.ensure(m + 1, st)); GEVC(A.sfill.ensure(m + 1, st)); GEVC(A.stgt.ensure(m + 1, st));
    GEVC(src.ensure(std::max<size_t>(p1 - p0, 1), st));
    HIPC(hipMemsetAsync(A.scnt.p, 0, w, st)); HIPC(hipMemsetAsync(A.sfill.p, 0, w, st));
    const unsigned nb = (unsigned)ceil_div(m, 256);
    hipLaunchKernelGGL(k_shuf_count, dim3(nb), dim3(256), 0, st, R, m, A.scnt);
    GEVC(scan_u32_on(st, c->d_sums, A.scnt, m, A.soff));
    hipLaunchKernelGGL(k_shuf_fill, dim3(nb), dim3(256), 0, st, R, m, A.soff, A.sfill, A.stgt);
    if (p1 > p0) hipLaunchKernelGGL(k_shuf_trace, dim3((unsigned)ceil_div(p1 - p0, 256)), dim3(256), 0, st, R, m, A.soff, A.stgt, p0, p1, src);
    KCHECK();
    return GEV_OK;
}
static u32 h_minstd_seed(u32 s) { const u32 x = s % GEV_M31; return x ? x : 1u; }
static int assort_mate(gev_ctx* c, int pop, const gev_assort_params* par, const uint32_t* seeds, const double* mating_value, const double* selection_value_func,
                       bool dev_sel, const int64_t* pedigree, gev_couple* couples_out, gev_assort_result* res, bool dev_records = false)
{
    GEVC(check_idx(c, pop, 0));
    if (!par || !seeds) return fail(GEV_EINVAL, "assort_mate: null params or seeds");
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "assort_mate: population %d has no current generation", pop);
    if (!dev_sel && !mating_value) return fail(GEV_EINVAL, "assort_mate: mating_value is NULL");
    const int dist = par->offspring_dist;
    const bool pois = dist == 'p' || dist == 'P', fixed = dist == 'f' || dist == 'F';
    if (!pois && !fixed) return fail(GEV_EINVAL, "assort_mate: offspring distribution '%c' is neither 'p' nor 'f'", (char)dist);
    const bool avoid = par->avoid_inbreeding != 0;
    const bool dev_ped = avoid && !pedigree && c->track_pedigree;      // the ids the library tracks itself (gev_set_track_pedigree)
    if (avoid && !pedigree && !dev_ped) return fail(GEV_EINVAL, "assort_mate: avoid_inbreeding needs the pedigree ids");
    if (dev_ped && !P.ids_ok) return fail(GEV_ESTATE, "assort_mate: population %d's pedigree ids were dropped when its rows changed (gev_upload_pedigree restores them)", pop);
    if (!std::isfinite(par->mat_cor)) return fail(GEV_EINVAL, "assort_mate: mat_cor is not finite");
    if (par->pop_size == 0 || par->pop_size >= 0x7fffffffull) return fail(GEV_EINVAL, "assort_mate: pop_size %llu out of range", (unsigned long long)par->pop_size);
    const size_t n_h = P.n_people;
    if (n_h == 0 || n_h >= 0x3fffffffull) return fail(GEV_EINVAL, "assort_mate: population of %zu individuals", n_h);
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    gev_ctx::AssortState& A = c->am;
    A.valid = false;
    gev_ctx::Scratch& sc = c->sc[c->gen_counter & 1];
    sc.mated = false;
    // father / mother of this scratch set were last read by the stitch two generations back
    GEVC(claim_scratch(c, sc, st, true, 0, false));
    const u32* logical = nullptr;
    if (!P.logical.empty()) {                                   // after a cross-GPU migration positions are not rows
        GEVC(upload_table(c, c->d_logical, P.logical.data(), n_h, st));
        logical = c->d_logical;
    }
    const double* d_mv; const double* d_svf = nullptr;
    if (dev_sel) { d_mv = P.d_sel[P.sbuf]; d_svf = d_mv + 2 * n_h; }
    else {
        GEVC(A.mv.ensure(n_h, st));
        HIPC(hipMemcpyAsync(A.mv.p, mating_value, n_h * sizeof(double), hipMemcpyHostToDevice, st));
        d_mv = A.mv;
        if (selection_value_func) {
            GEVC(A.svf.ensure(n_h, st));
            HIPC(hipMemcpyAsync(A.svf.p, selection_value_func, n_h * sizeof(double), hipMemcpyHostToDevice, st));
            d_svf = A.svf;
        }
    }
    const int64_t* d_ped = nullptr;
    if (avoid && !dev_ped) {
        GEVC(A.ped.ensure(n_h * 5, st));
        HIPC(hipMemcpyAsync(A.ped.p, pedigree, n_h * 5 * sizeof(int64_t), hipMemcpyHostToDevice, st));
        d_ped = A.ped;
    }
    const uint8_t* sex = P.d_sex[P.cur];
    const double mm = par->mm_percent;
    GEVC(A.stat.ensure(AMS_WORDS, st));
    HIPC(hipMemsetAsync(A.stat.p, 0, AMS_WORDS * sizeof(u32), st));
    u32* stat = A.stat;

    // :2184-2216 marriage draws: windows of start offsets per chunk, the chain over the chunks, one walk per chunk from its true start
    const u32 nc = (u32)ceil_div(n_h, AM_B);
    const double alpha = A.narrow_window ? 0.0 : 4.0;
    const u32 kmin = A.narrow_window ? 0u : 16u;
    const u32 wcap = (u32)round_up(2 * ((size_t)std::ceil(alpha * std::sqrt((double)n_h / 4.0)) + kmin + 1) + 1, 256);
    const u32 x_sel = h_minstd_seed(seeds[1]);
    GEVC(A.stats.ensure(nc, st)); GEVC(A.wlo.ensure(nc, st)); GEVC(A.ww.ensure(nc, st));
    GEVC(A.ends.ensure((size_t)nc * wcap, st)); GEVC(A.start.ensure(nc, st));
    GEVC(A.cm.ensure(n_h, st)); GEVC(A.cf.ensure(n_h, st));
    GEVC(A.om.ensure((n_h + 1), st)); GEVC(A.of.ensure((n_h + 1), st));
    GEVC(A.males.ensure(2 * n_h, st)); GEVC(A.females.ensure(2 * n_h, st));
    hipLaunchKernelGGL(k_am_chunk_stats, dim3(nc), dim3(256), 0, st, sex, logical, d_svf, n_h, A.stats);
    hipLaunchKernelGGL(k_am_windows, dim3(1), dim3(64), 0, st, A.stats, nc, alpha, kmin, wcap, A.wlo, A.ww);
    hipLaunchKernelGGL(k_am_walk, dim3(nc, wcap / 256), dim3(256), 0, st, sex, logical, d_svf, n_h, x_sel, mm, A.wlo, A.ww, wcap, A.ends);
    hipLaunchKernelGGL(k_am_chain, dim3(1), dim3(64), 0, st, sex, logical, d_svf, n_h, x_sel, mm, nc, A.wlo, A.ww, wcap,
                       A.ends, A.start, stat);
    hipLaunchKernelGGL(k_am_flags, dim3(nc), dim3(256), 0, st, sex, logical, d_svf, n_h, x_sel, mm, A.start, A.cm, A.cf);
    KCHECK();
    GEVC(scan_u32_on(st, c->d_sums, A.cm, n_h, A.om));
    GEVC(scan_u32_on(st, c->d_sums, A.cf, n_h, A.of));
    hipLaunchKernelGGL(k_am_compact, dim3((unsigned)ceil_div(n_h, 256)), dim3(256), 0, st, A.cm, A.cf, A.om,
                       A.of, n_h, A.males, A.females, stat);
    KCHECK();
    u32 h[AMS_WORDS];
    HIPC(hipMemcpyAsync(h, stat, sizeof h, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    const size_t nm = h[AMS_NM], nf = h[AMS_NF];
    A.n_chunks = nc; A.n_direct = h[AMS_NDIRECT]; A.pois_reruns = 0;
    gev_assort_result r = {nm, nf, 0, 0, 0};
    if (res) *res = r;
    const size_t n2 = std::min(nm, nf);
    if (n2 == 0) return fail(GEV_ENOMATE, "Error: couples=0, num_males_mate=%zu, num_females_mate=%zu", nm, nf);

    // :2232-2246 surplus removal: std::random_shuffle of the longer list on rand() after srand(seeds[0]), its first entries erased;
    // 'f' (:2340-2352) continues the same rand() stream (its remainder is known here unless inbred couples are left out)
    const size_t nL = std::max(nm, nf);
    const size_t n_rand_surplus = nL > n2 ? nL - 1 : 0;
    size_t n_rand = n_rand_surplus, remain_pre = 0;
    if (fixed && !avoid) {
        const size_t nfix = (size_t)std::floor((double)par->pop_size / (double)n2);
        remain_pre = par->pop_size - nfix * n2;
        if (remain_pre) n_rand += n2 - 1;
    }
    const GevRngTables* T = c->d_tables;
    if (n_rand) {
        GEVC(A.rnd.ensure(n_rand, st));
        hipLaunchKernelGGL(k_glibc_stream, dim3(1), dim3(64), 0, st, T, (u32)seeds[0], n_rand, A.rnd);
        KCHECK();
    }
    GEVC(A.kept.ensure(n2, st)); GEVC(A.sorted_m.ensure(n2, st)); GEVC(A.sorted_f.ensure(n2, st));
    const u32* list_m = A.males; const u32* list_f = A.females;
    if (nL > n2) {
        GEVC(am_shuffle(c, st, A.rnd, nL, nL - n2, nL, A.ssrc));
        hipLaunchKernelGGL(k_gather_u32, dim3((unsigned)ceil_div(n2, 256)), dim3(256), 0, st, nm > nf ? list_m : list_f, A.ssrc, n2, A.kept);
        KCHECK();
        if (nm > nf) list_m = A.kept; else list_f = A.kept;
    }
    // :2251-2252 both lists sorted by mating value (stable)
    GEVC(am_sort(c, st, d_mv, list_m, list_m, n2, A.sorted_m));
    GEVC(am_sort(c, st, d_mv, list_f, list_f, n2, A.sorted_f));

    // :2257-2285 the template: ras_mvnorm(n2, 0, [[1, c], [c, 1]]) = z * U (Eigen's LLT upper factor), ranked by CommFunc::ras_rank
    const double cc = par->mat_cor;
    const double x11 = 1.0 - (cc / 1.0) * (cc / 1.0);          // Eigen's unblocked LLT leaves A(1,1) = 1 at a non-positive pivot
    const double u01 = cc / 1.0, u11 = x11 > 0 ? std::sqrt(x11) : 1.0;
    const u64 n_cand = (u64)n2 + (u64)n2 * 3 / 10 + 4096;          // acceptance pi/4: n2 pairs need 1.273 n2 candidates on average
    const unsigned nbt = (unsigned)ceil_div((size_t)n_cand, POLAR_CHUNK);
    GEVC(A.tblk.ensure(nbt, st)); GEVC(A.t1.ensure(n2, st)); GEVC(A.t2.ensure(n2, st));
    GEVC(A.i1.ensure(n2, st)); GEVC(A.i2.ensure(n2, st));
    GEVC(A.pm.ensure(n2, st)); GEVC(A.pf.ensure(n2, st)); GEVC(A.inb.ensure(n2, st));
    GEVC(A.num.ensure(n2, st));
    const u32 x_tpl = h_minstd_seed(seeds[2]);
    hipLaunchKernelGGL(k_tpl_count, dim3(nbt), dim3(256), 0, st, x_tpl, n_cand, A.tblk);
    hipLaunchKernelGGL(k_tpl_emit, dim3(nbt), dim3(256), 0, st, x_tpl, n_cand, (u64)n2, A.tblk, u01, u11, A.t1, A.t2, stat);
    KCHECK();
    GEVC(am_sort(c, st, A.t1, nullptr, nullptr, n2, A.i1));
    GEVC(am_sort(c, st, A.t2, nullptr, nullptr, n2, A.i2));
    const unsigned nb2 = (unsigned)ceil_div(n2, 256);
    hipLaunchKernelGGL(k_am_couples, dim3(nb2), dim3(256), 0, st, A.i1, A.i2, A.sorted_m, A.sorted_f,
                       n2, A.pm, A.pf);
    if (dev_ped)
        hipLaunchKernelGGL(k_am_inbreed_ids, dim3(nb2), dim3(256), 0, st, A.pm, A.pf, n2, P.d_ids[P.ibuf],
                           P.ids_stride[P.ibuf], logical, A.inb, stat);
    else
        hipLaunchKernelGGL(k_am_inbreed, dim3(nb2), dim3(256), 0, st, A.pm, A.pf, n2, d_ped, A.inb, stat);
    KCHECK();
    size_t n_inb = 0;
    if (avoid) {
        HIPC(hipMemcpyAsync(h, stat, sizeof h, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        n_inb = h[AMS_NINB];
    }
    r.n_couples = n2; r.n_inbreed = n_inb;
    if (res) *res = r;
    const size_t n_ok = n2 - n_inb;
    if (n_ok == 0) return fail(GEV_EUNSUPPORTED, "assort_mate: all %zu couples are inbred (the reference divides by zero)", n2);

    // :2328-2355 offspring numbers, then the parents of every child in couple order
    GEVC(A.ocnt.ensure(n2, st)); GEVC(A.ooff.ensure((n2 + 1), st));
    size_t S = 0;
    double thr = 0;
    u32 L = 0;
    if (pois) {
        const double lam = (double)par->pop_size / (double)n_ok;
        if (!(lam < 12)) return fail(GEV_EUNSUPPORTED, "assort_mate: poisson_distribution with mean %g >= 12 (libstdc++'s rejection branch) is not supported", lam);
        thr = std::exp(-lam);
        S = A.short_poisson ? n2 / 2 + 16 : (size_t)((double)n2 * (lam + 1.0) * 1.15) + 4096;
        while ((n2 - 1) >> L) L++;                                     // levels: nxt^(2^j), j < L, cover every k < n2
    } else {
        const size_t nfix = (size_t)std::floor((double)par->pop_size / (double)n_ok);
        const size_t remain = par->pop_size - nfix * n_ok;
        if (avoid && remain) return fail(GEV_EUNSUPPORTED, "assort_mate: avoid_inbreeding with offspring_dist 'f' and %zu children left over (the reference indexes an empty list)", remain);
        hipLaunchKernelGGL(k_am_fill_i32, dim3(nb2), dim3(256), 0, st, A.num, n2, (int32_t)nfix);
        if (remain) {
            GEVC(am_shuffle(c, st, A.rnd + n_rand_surplus, n2, 0, remain, A.ssrc));
            hipLaunchKernelGGL(k_am_fixed_plus, dim3((unsigned)ceil_div(remain, 256)), dim3(256), 0, st, A.ssrc, remain, A.num);
        }
        KCHECK();
    }
    for (;;) {
        if (pois) {
            if (S >= 0xfffffff0ull) return fail(GEV_EDEVICE, "assort_mate: Poisson stream of %zu draws (internal error)", S);
            const size_t lv = std::max<u32>(L, 1);
            GEVC(A.pois.ensure(lv * (S + 1), st));
            u32* tabs = A.pois;
            const unsigned nbs = (unsigned)ceil_div(S + 1, 256);
            hipLaunchKernelGGL(k_pois_next, dim3(nbs), dim3(256), 0, st, h_minstd_seed(seeds[3]), (u64)S, thr, tabs);
            for (u32 j = 1; j < L; j++) hipLaunchKernelGGL(k_pois_double, dim3(nbs), dim3(256), 0, st, (const u32*)tabs + (size_t)(j - 1) * (S + 1), (u64)S, tabs + (size_t)j * (S + 1));
            hipLaunchKernelGGL(k_pois_start, dim3(nb2), dim3(256), 0, st, (const u32*)tabs, (u64)S, L, (u64)n2, A.num, stat);
            KCHECK();
        }
        hipLaunchKernelGGL(k_am_offspring_count, dim3(nb2), dim3(256), 0, st, A.num, A.inb, n2, A.ocnt);
        KCHECK();
        GEVC(scan_u32_on(st, c->d_sums, A.ocnt, n2, A.ooff));
        u32 tot = 0;
        HIPC(hipMemcpyAsync(h, stat, sizeof h, hipMemcpyDeviceToHost, st));
        HIPC(hipMemcpyAsync(&tot, A.ooff + n2, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        if (h[AMS_FLAGS] & AMF_TPL_SHORT) return fail(GEV_EDEVICE, "assort_mate: the template's candidate pairs ran out (internal error)");
        if (pois && (h[AMS_FLAGS] & AMF_POIS_SHORT)) {          // the stream ended inside a couple's draws: run it again, longer
            HIPC(hipMemsetAsync(stat + AMS_FLAGS, 0, sizeof(u32), st));
            S = 2 * S + 4096; A.pois_reruns++;
            continue;
        }
        r.n_offspring = tot;
        break;
    }
    if (res) *res = r;
    if (r.n_offspring) {
        GEVC(sc.father.ensure(r.n_offspring, st)); GEVC(sc.mother.ensure(r.n_offspring, st));
    }
    const bool records = couples_out || dev_records;           // dev_records: Couples_Info records left in d_couples (gev_generation_end copies them)
    if (records) GEVC(c->d_couples.ensure(n2, st));
    hipLaunchKernelGGL(k_am_expand, dim3(nb2), dim3(256), 0, st, A.pm, A.pf, A.num,
                       A.inb, A.ooff, n2, logical, r.n_offspring ? sc.father : nullptr,
                       r.n_offspring ? sc.mother : nullptr, records ? c->d_couples : nullptr);
    KCHECK();
    if (couples_out) HIPC(hipMemcpyAsync(couples_out, c->d_couples.p, n2 * sizeof(gev_couple), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    A.res = r; A.valid = true;
    if (r.n_offspring) { sc.mated = true; sc.mate_assort = true; sc.mate_pop = pop; sc.mate_n = r.n_offspring; sc.mate_epoch = P.layout_epoch; }
    return GEV_OK;
}
int gev_assort_mate(gev_ctx* c, int pop, const gev_assort_params* par, const uint32_t seeds[4], const double* mating_value,
                    const double* selection_value_func, const int64_t* pedigree, gev_couple* couples_out, gev_assort_result* res)
{
    return assort_mate(c, pop, par, seeds, mating_value, selection_value_func, false, pedigree, couples_out, res);
}
int gev_assort_mate_selected(gev_ctx* c, int pop, const gev_assort_params* par, const uint32_t seeds[4], const int64_t* pedigree,
                             gev_couple* couples_out, gev_assort_result* res)
{
    GEVC(check_selection(c, pop, "assort_mate_selected"));
    return assort_mate(c, pop, par, seeds, nullptr, nullptr, true, pedigree, couples_out, res);
}
int gev_last_assort_result(gev_ctx* c, gev_assort_result* res, gev_couple* couples_out)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (c->pend.active && (couples_out || !c->pend.assort))      // the counts of the assortative generation in flight may be read
        return fail(GEV_ESTATE, "last_assort_result: a generation is pending: call gev_generation_end / gev_reproduce_end first");
    gev_ctx::AssortState& A = c->am;
    if (!A.valid) return fail(GEV_ESTATE, "last_assort_result: no gev_assort_mate has completed on this context");
    if (res) *res = A.res;
    if (couples_out && A.res.n_couples) {
        HIPC(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const size_t n2 = A.res.n_couples;
        GEVC(c->d_couples.ensure(n2, st));
        hipLaunchKernelGGL(k_am_expand, dim3((unsigned)ceil_div(n2, 256)), dim3(256), 0, st, A.pm, A.pf, A.num,
                           A.inb, A.ooff, n2, (const u32*)nullptr, (u32*)nullptr, (u32*)nullptr, c->d_couples);
        KCHECK();
        HIPC(hipMemcpyAsync(couples_out, c->d_couples.p, n2 * sizeof(gev_couple), hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
    }
    return GEV_OK;
}
int gev_dbg_assort_knobs(gev_ctx* c, int narrow_window, int short_poisson)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    c->am.narrow_window = narrow_window != 0; c->am.short_poisson = short_poisson != 0;
    return GEV_OK;
}
int gev_dbg_assort_stats(gev_ctx* c, unsigned long long stats[3])
{
    if (!c || !stats) return fail(GEV_EINVAL, "null argument");
    stats[0] = c->am.n_chunks; stats[1] = c->am.n_direct; stats[2] = c->am.pois_reruns;
    return GEV_OK;
}
// One whole assortative generation: Simulation::assort_mate -> reproduce -> ras_compute_AD (sim_next_generation, :1907-1935, without
// --RM).  The mating seeds (3, or 4 with 'p') are drawn on the device from glob_state; gev_assort_mate runs with them (it waits for the
// list lengths, the inbred count with avoid_inbreeding, and the offspring count: n_offspring is random under 'p' and sizes everything
// after); then reproduce's 1 + n_offspring * nchr draws continue from the state behind the mating seeds, and the rest is enqueued as
// gev_generation_begin's is.  A head start queued by gev_set_generation_chain for a random-mating generation is dropped (it assumed
// other draws); none is queued behind an assortative generation.
static int generation_begin_assort(gev_ctx* c, int pop, uint32_t glob_state, const gev_assort_params* par, const double* mating_value,
                                   const double* selection_value_func, bool dev_sel, const int64_t* pedigree)
{
    GEVC(check_idx(c, pop, 0));
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "generation: population %d has no current generation (call gev_init_gen0)", pop);
    if (!par) return fail(GEV_EINVAL, "generation_begin_assort: null params");
    if (glob_state == 0 || glob_state >= GEV_M31) return fail(GEV_EINVAL, "generation: %u is not a state of std::minstd_rand0 (1 .. 2^31-2)", glob_state);
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    gev_ctx::Scratch& sc = c->sc[c->gen_counter & 1];
    // a head start for a random-mating generation must not write into the set any more, and is not used
    bool taken = false;
    GEVC(take_head_start(c, sc, HeadStart::NONE, pop, 0, false, 0u, nullptr, taken));
    // :2170, :2173, :2265 (and :2332 for 'p'): the mating seeds
    const bool pois = par->offspring_dist == 'p' || par->offspring_dist == 'P';
    uint32_t seeds[4] = {0, 0, 0, 0};
    uint32_t state = glob_state;
    GEVC(gev_glob_seeds(c, &state, pois ? 4 : 3, seeds));
    gev_assort_result r;
    GEVC(assort_mate(c, pop, par, seeds, mating_value, selection_value_func, dev_sel, pedigree, nullptr, &r, /*dev_records=*/true));
    const size_t n_people = r.n_offspring;
    GEVC(begin_prologue(c, pop, "generation", n_people, /*fused=*/true, nullptr, 0, 2 * sizeof(u32) + n_people + 16));
    gev_ctx::PendingRepro& q = c->pend;
    sc.mated = false;                                          // the couples are this generation's, not a later gev_reproduce's
    GEVC(claim_scratch(c, sc, st, true, n_people, q.has_mut));   // (father / mother already hold n_people entries: kept)
    GEVC(sc.globvals.ensure((2 + n_people * (size_t)c->nchr), st));
    q.glob_state = state;
    q.assort = true; q.assort_seed0 = seeds[0]; q.am_nm = r.num_males_mate; q.am_nf = r.num_females_mate; q.am_couples = r.n_couples;
    q.cidx_mode = 2; q.n_couples = r.n_couples;
    GEVC(enqueue_attempt(c, 0));
    q.active = true;
    return GEV_OK;
}
int gev_generation_begin_assort(gev_ctx* c, int pop, uint32_t glob_state, const gev_assort_params* par, const double* mating_value,
                                const double* selection_value_func, const int64_t* pedigree)
{
    if (!mating_value) return fail(GEV_EINVAL, "generation_begin_assort: mating_value is NULL");
    return generation_begin_assort(c, pop, glob_state, par, mating_value, selection_value_func, false, pedigree);
}
int gev_generation_begin_assort_selected(gev_ctx* c, int pop, uint32_t glob_state, const gev_assort_params* par, const int64_t* pedigree)
{
    GEVC(check_selection(c, pop, "generation_begin_assort_selected"));
    return generation_begin_assort(c, pop, glob_state, par, nullptr, nullptr, true, pedigree);
}
// Simulation::ras_glob_seed (src/Simulation.cpp:17-21) called n times, evaluated on the device: *engine_state = the state of
// glob_generator (std::minstd_rand0) before, and after on return; out (host, n values) may be NULL.
int gev_glob_seeds(gev_ctx* c, uint32_t* engine_state, size_t n, uint32_t* out)
{
    if (!c || !engine_state) return fail(GEV_EINVAL, "glob_seeds: null argument");
    if (c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first");
    if (*engine_state == 0 || *engine_state >= GEV_M31) return fail(GEV_EINVAL, "glob_seeds: %u is not a state of std::minstd_rand0 (1 .. 2^31-2)", *engine_state);
    if (n == 0) return GEV_OK;
    if (n >= 0x7fffffffull) return fail(GEV_EINVAL, "glob_seeds: too many values");
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    GEVC(c->d_tmp.ensure((n + 4) * sizeof(u32), st));
    u32* vals = c->d_tmp.as<u32>() + 4; u32* stat = c->d_tmp.as<u32>();       // stat = {state, flags}
    HIPC(hipMemsetAsync(stat, 0, 16, st));
    GEVC(enqueue_glob(c->mate.globblk, st, *engine_state, nullptr, n, vals, stat, stat + 1));
    u32 h[2] = {0, 0};
    HIPC(hipMemcpyAsync(h, stat, sizeof h, hipMemcpyDeviceToHost, st));
    if (out) HIPC(hipMemcpyAsync(out, vals, n * sizeof(u32), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (h[1]) return fail(GEV_EDEVICE, "glob_seeds: the rejection stream ran out of candidates (internal error)");
    *engine_state = h[0];
    return GEV_OK;
}
// The sexes of the generation whose sampling gev_presample has enqueued (they come out of the rand() chain of the sampling
// kernels, src/Simulation.cpp:2472, and need nothing else): lets a host that mates at random form the NEXT couples while the
// device still works on this generation.  Waits for the sampling kernels only.
int gev_presample_sex(gev_ctx* c, int pop, uint8_t* sex_out, size_t n_people)
{
    GEVC(check_idx(c, pop, 0));
    if (!sex_out) return fail(GEV_EINVAL, "presample_sex: null output");
    gev_ctx::Scratch& sc = c->sc[c->gen_counter & 1];
    const HeadStart& h = sc.hs;
    const bool ours = h.kind == HeadStart::PRESAMPLE && h.pop == pop && h.n_people == n_people;
    if (ours && h.dropped)       // by a redo of the previous generation (larger record regions): sample again from the retained inputs
        GEVC(gev_presample(c, pop, h.seed, h.has_mut ? (const uint32_t*)c->h_seeds.p : nullptr, h.has_mut ? n_people * (size_t)c->nchr : 0, n_people));
    if (!ours || h.dropped) return fail(GEV_ESTATE, "presample_sex: no matching gev_presample is pending");
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->serialize ? c->stream : c->stream_samp;
    HIPC(hipMemcpyAsync(sex_out, sc.sex.p, n_people, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
// Enqueue the sampling kernels of the NEXT gev_reproduce of `pop` now (they need the seeds and the offspring count, not the
// couples) and return at once: the host can form the couples while the GPU samples.  gev_reproduce recognises the
// same (seed, mutation seeds, n_people) and skips its own sampling; anything else simply samples again.
int gev_presample(gev_ctx* c, int pop, uint32_t seed_reproduce, const uint32_t* mut_seeds, size_t n_mut_seeds, size_t n_people)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (pop < 0 || pop >= c->n_pop) return fail(GEV_EINVAL, "population index %d out of range", pop);   // (allowed between gev_reproduce_begin and _end)
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "presample: population %d has no current generation (call gev_init_gen0)", pop);
    HIPC(hipSetDevice(c->device));
    const size_t T = n_people * (size_t)c->nchr;
    const bool has_mut = mut_seeds != nullptr;
    GEVC(check_sizes(c, "presample", n_people, mut_seeds, n_mut_seeds));
    GEVC(finalize_static(c, pop));
    hipStream_t st = c->serialize ? c->stream : c->stream_samp;   // the head start has a stream of its own: it runs next to the lists / A-D of the generation in flight
    // the scratch set of the generation AFTER the one in flight when called between gev_reproduce_begin and _end
    gev_ctx::Scratch& sc = c->sc[(c->gen_counter + (c->pend.active ? 1u : 0u)) & 1];
    drop_head_start(sc);                                 // whatever the set held is overwritten (same stream: behind it)
    if (has_mut && mut_seeds != (const uint32_t*)c->h_seeds.p) {
        GEVC(c->h_seeds.ensure(T * sizeof(u32), T * sizeof(u32) * 5 / 4 + 4096, st));   // an earlier copy out of the old buffer may be in flight
        memcpy(c->h_seeds.p, mut_seeds, T * sizeof(u32));
    }
    // Called while a generation is in flight, the stitch that last used this scratch set may still be running: nothing here waits
    // for it on the host; the sampling stream does.
    GEVC(claim_scratch(c, sc, st, !c->pend.active, n_people, has_mut));
    if (has_mut) HIPC(hipMemcpyAsync(sc.mutseeds.p, c->h_seeds.p, T * sizeof(u32), hipMemcpyHostToDevice, st));
    GEVC(enqueue_sampling(c, sc, pop, n_people, has_mut, seed_reproduce, st));
    HIPC(hipEventRecord(sc.ev[EV_SAMPLED], st));
    sc.hs.kind = HeadStart::PRESAMPLE; sc.hs.dropped = false; sc.hs.pop = pop; sc.hs.n_people = n_people; sc.hs.has_mut = has_mut; sc.hs.seed = seed_reproduce;
    return GEV_OK;
}
// wait for all device work of the context (every stream) and collect pending kernel timings
int gev_sync(gev_ctx* c)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first");
    HIPC(hipSetDevice(c->device));
    for (Stream& s : c->streams) HIPC(hipStreamSynchronize(s));
    for (auto& sc : c->sc) { GEVC(harvest_timing(c, sc)); sc.stitch_pending = false; }
    c->planes_pending = false;
    if (g_graveyard.bytes) g_graveyard.drain(c->device, false);
    return GEV_OK;
}
// what the dense stitch wrote, summed over all gev_reproduce calls and active chromosomes: bytes written and bytes of the rows
// of the generations produced (the difference = row segments without a crossover boundary, which share the parental unit),
// and the same in segments
int gev_stitch_totals(gev_ctx* c, unsigned long long* bytes_written, unsigned long long* bytes_total, unsigned long long* segments_written, unsigned long long* segments_total)
{
    if (!c || !bytes_written || !bytes_total) return fail(GEV_EINVAL, "null");
    *bytes_written = 16ull * c->chunks_written_sum; *bytes_total = 16ull * c->chunks_total_sum;
    if (segments_written) *segments_written = c->segments_written_sum;
    if (segments_total) *segments_total = c->segments_total_sum;
    return GEV_OK;
}
// cumulative kernel time per phase over all harvested generations: sampling, dense stitch, sparse, sum
int gev_timing_totals(gev_ctx* c, double ms_sum[4], unsigned long long* n_generations)
{
    if (!c || !ms_sum || !n_generations) return fail(GEV_EINVAL, "null");
    GEVC(gev_sync(c));
    for (int i = 0; i < 4; i++) ms_sum[i] = c->ms_sum[i];
    *n_generations = c->ms_count;
    return GEV_OK;
}

// ---- Simulation::ras_compute_AD -----------------------------------------------------------
// kernels of ras_compute_AD on buffer set `buf` (current generation, or the one being produced)
// the A/D kernel of a population: one root population (or shared effects) and the block's rows fit LDS: the term-table kernels,
// the wide one when every CV file is in position order and the allele sub-rows are whole 16-byte chunks; else per haplotype
static int choose_ad_path(const gev_ctx* c, int pop, int* ipb_out, bool* skip_d_out)
{
    const PopState& P = c->pop[pop];
    u32 sub_max = 0; bool all_have_cv = true, any = false;
    bool direct = true;                                      // every CV file in position order: rows are read from global memory, no row staging
    bool chunked = true, skip_d = true;                      // ... their allele sub-rows in whole 16-byte chunks: the terms in few large pieces (k_ad_accumulate_wide)
    for (int p = 0; p < c->nphen; p++)
        for (int k = 0; k < c->nchr; k++) {
            if (!c->chr_active[k]) continue;
            const CvStatic& V = P.cv[p][k];
            any = true; sub_max = std::max(sub_max, V.sub_w32); all_have_cv &= V.C > 0;
            direct &= V.cols_sorted;
            // (or the row stride pads the sub-row to whole chunks: the piece's 16-byte reads stay inside the row)
            const bool whole = (V.stride_w32 & 3u) == 0 && ((V.sub_w32 & 3u) == 0 || V.stride_w32 == round_up((size_t)V.sub_w32, 4));
            chunked &= whole && V.C > 0 && (size_t)V.stride_w32 * 32 >= (((size_t)V.C + 127) & ~(size_t)127);
            skip_d &= V.vd == 0;
        }
    const u32 S1 = sub_max | 1u;
    int ipb = 0;
    const size_t ad_tab_lds = AD_CHUNK * 4 + AD_CHUNK * 6 * 8 + 8;          // column + table chunk behind the rows
    if ((c->rp_bits == 0 || c->ad_effects_shared) && all_have_cv) { for (int cand : {256, 128, 64}) if ((size_t)2 * cand * S1 * 4 + ad_tab_lds <= 64 * 1024) { ipb = cand; break; } }
    if (ipb_out) *ipb_out = ipb;
    if (skip_d_out) *skip_d_out = skip_d;
    if (!any) return AD_PATH_NONE;
    if (ipb) return direct && chunked ? AD_PATH_WIDE : direct ? AD_PATH_TAB_DIRECT : AD_PATH_TAB;
    // several root populations with their own CV effects: the piecewise kernel when every CV file is in position order
    return direct && c->rp_bits >= 1 && c->rp_bits <= 3 && !c->ad_no_rp ? AD_PATH_RP : AD_PATH_GENERAL;
}
// counts: AD_COUNTS_PARTIAL: the allele counts of the CV columns were accumulated by k_stitch_small while it wrote the planes;
// AD_COUNTS_DONE: k_cv_newmut_sum has also added them up and reset the NaN flag (only in front of k_ad_accumulate_wide)
// hbuf: the pinned result buffer (default: the published generation's)
static int enqueue_ad(gev_ctx* c, int pop, int buf, size_t n, int counts, int hbuf)
{
    if (hbuf < 0) hbuf = (int)((c->gen_counter + 1) & 1);
    PopState& P = c->pop[pop];
    hipStream_t st = c->stream;
    const size_t rows = 2 * n;
    const int nchr = c->nchr, nphen = c->nphen;
    GEVC(c->d_addchr.ensure(n * nchr * nphen, st)); GEVC(c->d_domchr.ensure(n * nchr * nphen, st));
    GEVC(c->d_add.ensure(n * nphen, st)); GEVC(c->d_dom.ensure(n * nphen, st));
    GEVC(c->d_flag.ensure(16, st));
    if (!c->d_cvdone.p) { GEVC(c->d_cvdone.ensure((size_t)nchr * nphen, st)); HIPC(hipMemsetAsync(c->d_cvdone.p, 0, (size_t)nchr * nphen * sizeof(u32), st)); }   // block tickets of k_cv_finish / k_ad_accumulate_wide (they re-zero themselves)
    c->ad_host_set_pop = -1;                                 // d_add / d_dom are rewritten below: totals handed in by gev_set_ad are gone
    if (c->any_inactive) {                                   // chromosomes held elsewhere contribute exact zeros here
        HIPC(hipMemsetAsync(c->d_addchr.p, 0, n * nchr * nphen * sizeof(double), st)); HIPC(hipMemsetAsync(c->d_domchr.p, 0, n * nchr * nphen * sizeof(double), st));
    }
    // one table entry per (phenotype, active chromosome); every kernel below covers all of them in one launch
    std::vector<AdWork> aw;
    u32 c_max = 0, sub_max = 0;
    for (int p = 0; p < nphen; p++)
        for (int k = 0; k < nchr; k++) {
            if (!c->chr_active[k]) continue;
            CvStatic& V = P.cv[p][k];
            c_max = std::max(c_max, V.C); sub_max = std::max(sub_max, V.sub_w32);
        }
    const u32 S1 = sub_max | 1u;
    int ipb = 0; bool skip_d = true;
    const size_t ad_tab_lds = AD_CHUNK * 4 + AD_CHUNK * 6 * 8 + 8;          // column + table chunk behind the rows
    const int path = choose_ad_path(c, pop, &ipb, &skip_d);
    if (counts == AD_COUNTS_DONE && path != AD_PATH_WIDE) return fail(GEV_ESTATE, "enqueue_ad: summed column counts in front of A/D path %d", path);
    for (int p = 0; p < nphen; p++)
        for (int k = 0; k < nchr; k++) {
            if (!c->chr_active[k]) continue;
            CvStatic& V = P.cv[p][k]; ChrStatic& S = P.cs[k];
            if (ipb) GEVC(V.d_tab.ensure((size_t)V.C * 6, st));
            AdWork a{};
            a.cvp = P.cvp[p][k][buf];
            a.pos_sorted = V.d_pos_sorted; a.pos_file = V.d_pos_file; a.col_of_icv = V.d_col_of_icv;
            a.a = V.d_a; a.d = V.d_d; a.aptr = V.d_aptr; a.dptr = V.d_dptr;
            a.counts = V.d_counts; a.frq = V.d_frq; a.tab = ipb ? V.d_tab : nullptr;
            a.add_out = c->d_addchr + (size_t)k * nphen + p; a.dom_out = c->d_domchr + (size_t)k * nphen + p;
            const bool one_chr = nchr == 1;                                     // the sum over chromosomes is 0 + x: written with the per-chromosome value
            a.add_tot = one_chr ? c->d_add + p : nullptr; a.dom_tot = one_chr ? c->d_dom + p : nullptr;
            a.partial = counts == AD_COUNTS_PARTIAL ? V.d_partial : nullptr;
            a.bp0 = S.rbp.front(); a.bp_end = S.rbp.back(); a.vd = V.vd;
            a.stride_w32 = V.stride_w32; a.sub_w32 = V.sub_w32; a.C = V.C; a.own_pop = pop; a.cols_sorted = V.cols_sorted ? 1u : 0u;
            aw.push_back(a);
        }
    const unsigned nw = (unsigned)aw.size();
    if (nw) {
        Dev<AdWork>& adw = c->d_adwork2[hbuf]; std::vector<uint8_t>& adw_shadow = c->adwork_shadow[hbuf];      // (one table per result buffer: they alternate with the generations)
        GEVC(upload_table_cached(c, adw, adw_shadow, aw.data(), aw.size(), st));
        const AdWork* At = adw;
        const size_t out_stride = (size_t)nchr * nphen, tot_stride = (size_t)nphen;
        u32* flag = c->d_flag.as<u32>();
        if (c_max && counts == AD_COUNTS_NONE) {
            const unsigned gy = (unsigned)std::min<size_t>(std::max<size_t>(rows / 512, 1), 256);
            hipLaunchKernelGGL(k_cv_count, dim3((unsigned)ceil_div(c_max, 256), gy, nw), dim3(256), 0, st, At, rows);
        }
        // counts -> frequencies (+ the term table of the fast path), NaN flag reset: one launch -- none behind k_cv_newmut_sum, where
        // the counts are complete, the flag is reset and k_ad_accumulate_wide computes frequencies and terms itself
        const unsigned nblk = counts == AD_COUNTS_PARTIAL ? (unsigned)ceil_div(rows, SMALL_ROWS_PER_BLOCK) : 0u;
        if (counts != AD_COUNTS_DONE) hipLaunchKernelGGL(k_cv_finish, dim3((unsigned)std::max<size_t>(ceil_div(c_max, 256), 1), nblk ? std::min((nblk + 7u) / 8u, 128u) : 1u, nw), dim3(256), 0, st, At, nblk, n, c->d_cvdone, flag);
        if (ipb) {
            if (path == AD_PATH_WIDE) {
                const unsigned nb = (unsigned)ceil_div(n, 256);
                u32* done = c->d_cvdone;
                if (counts == AD_COUNTS_DONE) {
                    if (skip_d) hipLaunchKernelGGL((k_ad_accumulate_wide<true, true>), dim3(nb, nw), dim3(256), 0, st, At, n, out_stride, tot_stride, flag, done);
                    else hipLaunchKernelGGL((k_ad_accumulate_wide<false, true>), dim3(nb, nw), dim3(256), 0, st, At, n, out_stride, tot_stride, flag, done);
                } else if (skip_d) hipLaunchKernelGGL((k_ad_accumulate_wide<true, false>), dim3(nb, nw), dim3(256), 0, st, At, n, out_stride, tot_stride, flag, done);
                else hipLaunchKernelGGL((k_ad_accumulate_wide<false, false>), dim3(nb, nw), dim3(256), 0, st, At, n, out_stride, tot_stride, flag, done);
            } else if (path == AD_PATH_TAB_DIRECT) {
                const unsigned nb = (unsigned)ceil_div(n, 256);
                hipLaunchKernelGGL((k_ad_accumulate_tab<256>), dim3(nb, nw), dim3(256), ad_tab_lds, st, At, 0u, n, out_stride, tot_stride, flag, 1);
            } else {
                const size_t lds = (size_t)2 * ipb * S1 * 4 + ad_tab_lds;
                const unsigned nb = (unsigned)ceil_div(n, ipb);
                if (ipb == 256) hipLaunchKernelGGL((k_ad_accumulate_tab<256>), dim3(nb, nw), dim3(256), lds, st, At, S1, n, out_stride, tot_stride, flag, 0);
                else if (ipb == 128) hipLaunchKernelGGL((k_ad_accumulate_tab<128>), dim3(nb, nw), dim3(128), lds, st, At, S1, n, out_stride, tot_stride, flag, 0);
                else hipLaunchKernelGGL((k_ad_accumulate_tab<64>), dim3(nb, nw), dim3(64), lds, st, At, S1, n, out_stride, tot_stride, flag, 0);
            }
        } else {
            // several root populations with their own CV effects: the piecewise kernel when every CV file is in position order
            const bool rp = path == AD_PATH_RP;
            const dim3 grid((unsigned)ceil_div(n, 256), nw);
            const size_t lds = (size_t)ADRP_PIECE * ((size_t)c->n_pop * 2 + 5) * sizeof(double);
            if (rp && c->rp_bits == 1) hipLaunchKernelGGL((k_ad_accumulate_rp<1>), grid, dim3(256), lds, st, At, (u32)c->n_pop, n, out_stride, tot_stride, flag);
            else if (rp && c->rp_bits == 2) hipLaunchKernelGGL((k_ad_accumulate_rp<2>), grid, dim3(256), lds, st, At, (u32)c->n_pop, n, out_stride, tot_stride, flag);
            else if (rp && c->rp_bits == 3) hipLaunchKernelGGL((k_ad_accumulate_rp<3>), grid, dim3(256), lds, st, At, (u32)c->n_pop, n, out_stride, tot_stride, flag);
            else hipLaunchKernelGGL(k_ad_accumulate, grid, dim3(256), 0, st, At, c->rp_bits, n, out_stride, tot_stride, flag);
        }
        KCHECK();
        c->ad_path = path | (counts == AD_COUNTS_DONE ? AD_PATH_FROM_COUNTS : 0);
    } else HIPC(hipMemsetAsync(c->d_flag.p, 0xff, 4, st));
    if (nchr > 1 || !nw) {                                   // one chromosome: the A/D kernels wrote the totals themselves
        hipLaunchKernelGGL(k_ad_sum_chr, dim3((unsigned)ceil_div(n * nphen, 256)), dim3(256), 0, st, c->d_addchr, c->d_domchr, c->d_add, c->d_dom, n, nchr, nphen);
        KCHECK();
    }
    // results to the pinned host cache: [flag | additive | dominance].  The per-chromosome arrays stay on the device and are
    // copied when gev_compute_ad is asked for them.  vd == 0 for every phenotype: the reference zeroes d (:2698-2699), every
    // D-term is (+-0) * ... and the running sums stay +0.0 exactly -- nothing to copy, gev_compute_ad fills zeros.
    const size_t nd = n * nphen;
    const size_t bytes = 16 + 2 * nd * sizeof(double);
    GEVC(c->h_ad2[hbuf].ensure(bytes, bytes * 5 / 4 + 4096, st));    // (copies into the old buffer may be in flight on this stream)
    bool dom_zero = true;
    for (const AdWork& a : aw) dom_zero &= a.vd == 0;
    c->ad_dom_zero2[hbuf] = dom_zero;
    uint8_t* h = (uint8_t*)c->h_ad2[hbuf].p;
    HIPC(hipMemcpyAsync(h, c->d_flag.p, 4, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(h + 16, c->d_add.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (!dom_zero) HIPC(hipMemcpyAsync(h + 16 + nd * 8, c->d_dom.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    return GEV_OK;
}
int gev_compute_ad(gev_ctx* c, int pop, double* additive, double* dominance, double* add_chr, double* dom_chr)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (pop < 0 || pop >= c->n_pop) return fail(GEV_EINVAL, "population index %d out of range", pop);
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "compute_ad: population %d has no current generation", pop);
    const int nchr = c->nchr, nphen = c->nphen;
    const int hb = (int)((c->gen_counter + 1) & 1);          // the published generation's result buffer
    if (c->pend.active) {
        // a generation is in flight: the CURRENT generation's values can still be handed out if they were computed with it (they
        // sit in the other pinned buffer); anything that needs device work has to wait for gev_reproduce_end / gev_generation_end
        if (c->ad_cached_pop != pop || add_chr || dom_chr)
            return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first");
    } else {
        HIPC(hipSetDevice(c->device));
        if (!c->multipop_ready) GEVC(check_multipop(c));
        GEVC(materialize_order(c, pop));
        if (c->ad_cached_pop != pop) {          // not computed eagerly by the last gev_reproduce of this population
            GEVC(enqueue_ad(c, pop, P.cur, P.n_people));
            HIPC(hipStreamSynchronize(c->stream));
            c->ad_cached_pop = pop;
            for (int p = 0; p < nphen; p++) for (int k = 0; k < nchr; k++) P.cv[p][k].frq_valid = true;
        }
    }
    const size_t n = P.n_people;
    const uint8_t* h = (const uint8_t*)c->h_ad2[hb].p;
    const size_t nd = n * nphen, ndc = n * (size_t)nchr * nphen;
    const u32 flag = *(const u32*)h;
    if (additive) memcpy(additive, h + 16, nd * sizeof(double));
    if (dominance) { if (c->ad_dom_zero2[hb]) memset(dominance, 0, nd * sizeof(double)); else memcpy(dominance, h + 16 + nd * 8, nd * sizeof(double)); }
    if (add_chr || dom_chr) {                                // (the arrays of the generation's A/D kernels are still in place: any later A/D run resets ad_cached_pop)
        if (add_chr) HIPC(hipMemcpyAsync(add_chr, c->d_addchr.p, ndc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (dom_chr) HIPC(hipMemcpyAsync(dom_chr, c->d_domchr.p, ndc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    if (flag != 0xffffffffu) return fail(GEV_ENAN, "Error: A or D is nan for human %u", flag);
    return GEV_OK;
}
int gev_compute_ad_device(gev_ctx* c, int pop, double** add_chr, double** dom_chr, size_t* n_doubles)
{
    GEVC(check_idx(c, pop, 0));
    GEVC(check_not_pending(c));
    if (!add_chr || !dom_chr || !n_doubles) return fail(GEV_EINVAL, "compute_ad_device: null argument");
    GEVC(gev_compute_ad(c, pop, nullptr, nullptr, nullptr, nullptr));          // (computes unless the last generation already did; checks the NaN flag)
    PopState& P = c->pop[pop];
    *add_chr = c->d_addchr; *dom_chr = c->d_domchr; *n_doubles = P.n_people * (size_t)c->nchr * c->nphen;
    return GEV_OK;
}
int gev_ad_finish_device(gev_ctx* c, int pop, double* additive, double* dominance, double* add_chr_out, double* dom_chr_out)
{
    GEVC(check_idx(c, pop, 0));
    GEVC(check_not_pending(c));
    PopState& P = c->pop[pop];
    if (!P.gen0 || c->ad_cached_pop != pop) return fail(GEV_ESTATE, "ad_finish_device: call gev_compute_ad_device for population %d first", pop);
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t n = P.n_people; const int nchr = c->nchr, nphen = c->nphen;
    const size_t nd = n * nphen, ndc = nd * nchr;
    GEVC(c->d_add.ensure(nd, st)); GEVC(c->d_dom.ensure(nd, st));
    hipLaunchKernelGGL(k_ad_sum_chr, dim3((unsigned)ceil_div(n * nphen, 256)), dim3(256), 0, st, c->d_addchr, c->d_domchr, c->d_add, c->d_dom, n, nchr, nphen);
    KCHECK();
    if (additive) HIPC(hipMemcpyAsync(additive, c->d_add.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (dominance) HIPC(hipMemcpyAsync(dominance, c->d_dom.p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    if (add_chr_out) HIPC(hipMemcpyAsync(add_chr_out, c->d_addchr.p, ndc * sizeof(double), hipMemcpyDeviceToHost, st));
    if (dom_chr_out) HIPC(hipMemcpyAsync(dom_chr_out, c->d_domchr.p, ndc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    c->ad_host_set_pop = pop;                                  // the totals in d_add / d_dom are the population's (as after gev_set_ad); the pinned cache holds this context's share only
    c->ad_cached_pop = -1;
    return GEV_OK;
}
// ---- Simulation::ras_scale_AD_compute_GEF ---------------------------------
// The normal streams and the mean / variance sums of this call, of gev_compute_selection and of gev_generation_phenotypes
// (gev_normal.h).  Their scratch (c->ph.streams / blk / partial) is shared: every caller enqueues on c->stream.  The status words
// (stream offsets, short flag) and the statistics belong to the caller.
static size_t ph_candidates(const gev_ctx* c, size_t n, int shift)
{
    if (c->ph.short_candidates && shift == 0) return n / 4 + 16;
    return ((size_t)((n / 2 + 1) / 0.7) + 4096) << shift;                        // acceptance = pi/4
}
// mean / var of nvec vectors into stats (k_ph_var_partial / _final, both passes)
static int ph_var(gev_ctx* c, const double* base, size_t vec_stride, size_t elem_stride, size_t n, unsigned nvec, double* stats)
{
    hipStream_t st = c->stream;
    GEVC(c->ph.partial.ensure((size_t)nvec * 256, st));
    const int nb = (int)std::min<size_t>(ceil_div(n, 256), 256);
    for (int pass = 0; pass < 2; pass++) {
        hipLaunchKernelGGL(k_ph_var_partial, dim3(nb, nvec), dim3(256), 0, st, base, vec_stride, elem_stride, n, (const double*)stats, pass, c->ph.partial);
        hipLaunchKernelGGL(k_ph_var_final, dim3(nvec), dim3(256), 0, st, c->ph.partial, nb, n, pass, stats);
    }
    KCHECK();
    return GEV_OK;
}
// one batch of streams: *flag |= NRM_CAND_SHORT when one of them ran out of candidate pairs
static int ph_streams(gev_ctx* c, std::vector<NrmStream>& v, const u32* seeds, u32* starts, u32* flag)
{
    if (v.empty()) return GEV_OK;
    hipStream_t st = c->stream;
    u32 off = 0, nb_max = 0;
    for (NrmStream& s : v) { s.n_blocks = (u32)ceil_div((size_t)s.n_cand, POLAR_CHUNK); s.blk_off = off; off += s.n_blocks; nb_max = std::max(nb_max, s.n_blocks); }
    GEVC(c->ph.blk.ensure(off, st));
    GEVC(upload_table(c, c->ph.streams, v.data(), v.size(), st));
    hipLaunchKernelGGL(k_nrm_count, dim3(nb_max, (unsigned)v.size()), dim3(256), 0, st, c->ph.streams, seeds, (const u32*)starts, c->ph.blk);
    hipLaunchKernelGGL(k_nrm_emit, dim3(nb_max, (unsigned)v.size()), dim3(256), 0, st, c->ph.streams, seeds, starts, c->ph.blk, flag);
    KCHECK();
    return GEV_OK;
}
enum { GEF_FLAG = 0, GEF_STARTS = 1, GEF_WORDS = 4 };       // gef.stat: the short flag, the stream offsets (unused: no stream continues another), then {mean, var} of e
int gev_scale_ad_compute_gef(gev_ctx* c, int pop, int phen, const gev_gef_params* par, uint32_t seed,
                             const double* common_sibling, const double* f_father, const double* f_mother,
                             double* additive, double* dominance, double* bv, double* e_noise, double* parental_effect, double* phen_out)
{
    GEVC(check_idx(c, pop, 0, phen));
    if (c->any_inactive && c->ad_host_set_pop != pop)
        return fail(GEV_ESTATE, "scale_ad_compute_gef: this context holds a subset of the chromosomes: give it the all-reduced raw A/D first (gev_set_ad)");
    if (!par) return fail(GEV_EINVAL, "scale_ad_compute_gef: null parameters");
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "scale_ad_compute_gef: population %d has no current generation", pop);
    HIPC(hipSetDevice(c->device));
    if (c->ad_cached_pop != pop && c->ad_host_set_pop != pop) GEVC(gev_compute_ad(c, pop, nullptr, nullptr, nullptr, nullptr));      // raw A/D of this generation on the device
    hipStream_t st = c->stream;
    const size_t n = P.n_people;
    GEVC(c->gef.io.ensure(10 * n, st));
    double* io = c->gef.io;
    double *d_e = io, *d_par = io + n, *d_cs = io + 2 * n, *d_ff = io + 3 * n, *d_out = io + 4 * n;     // d_out: 6 vectors
    GEVC(c->gef.stat.ensure(GEF_WORDS * sizeof(u32) + 2 * sizeof(double), st));
    u32* stat = c->gef.stat.as<u32>(); double* e_stats = (double*)(stat + GEF_WORDS);
    const bool need_par = par->vf > 0;
    if (par->gen_num != 0 && need_par) {
        double* d_fm = d_out;                                                                             // staging before d_out is written
        if (f_father) HIPC(hipMemcpyAsync(d_ff, f_father, n * sizeof(double), hipMemcpyHostToDevice, st));
        if (f_mother) HIPC(hipMemcpyAsync(d_fm, f_mother, n * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_par_eff, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, f_father ? d_ff : (const double*)nullptr, f_mother ? d_fm : (const double*)nullptr, n, par->beta, d_par);
        KCHECK();
        HIPC(hipStreamSynchronize(st));
    }
    if (common_sibling) HIPC(hipMemcpyAsync(d_cs, common_sibling, n * sizeof(double), hipMemcpyHostToDevice, st));
    double s_a = 1;
    if (par->va > 0) s_a = std::sqrt(par->s2_a_gen0 / par->va);
    double s_d = 0;
    if (par->vd > 0) s_d = std::sqrt(par->s2_d_gen0 / par->vd); else if (par->vd == -1) s_d = 1;
    Dev<double>& keep = P.d_phen[P.sbuf];                                                                     // the population's phenotypes, for gev_compute_selection
    GEVC(keep.ensure(n * (size_t)c->nphen, st, /*keep=*/true));
    double* outs[6] = {additive, dominance, bv, e_noise, parental_effect, phen_out};
    // the streams, var(e), the scaling and the copies out, with twice the candidate pairs while a stream runs short of them
    // (practically never: acceptance far below pi/4)
    for (int attempt = 0; attempt < 4; attempt++) {
        if (attempt) c->ph.reruns++;
        HIPC(hipMemsetAsync(stat, 0, GEF_WORDS * sizeof(u32), st));
        std::vector<NrmStream> batch;
        NrmStream e{}; e.seed_idx = -1; e.seed_val = seed; e.start_idx = e.next_idx = -1; e.n = n; e.n_cand = ph_candidates(c, n, attempt); e.sd = 1.0; e.out = d_e;
        batch.push_back(e);                                                                               // generator_e(seed), N(0,1), :3080-3102
        if (par->gen_num == 0 && need_par) { NrmStream f = e; f.seed_add = 1; f.sd = std::sqrt(par->vf); f.out = d_par; batch.push_back(f); }   // generator_f(seed+1), :3095-3114
        GEVC(ph_streams(c, batch, nullptr, stat + GEF_STARTS, stat + GEF_FLAG));
        GEVC(ph_var(c, d_e, n, 1, n, 1, e_stats));                                                        // CommFunc::var(e): two passes, n-1
        hipLaunchKernelGGL(k_gef_apply, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, c->d_add + phen, c->d_dom + phen, (size_t)c->nphen,
                           d_e, (const double*)e_stats, d_par, common_sibling ? d_cs : (const double*)nullptr, n, s_a, s_d, par->ve, par->vf,
                           d_out, d_out + n, d_out + 2 * n, d_out + 3 * n, d_out + 4 * n, d_out + 5 * n, keep + phen);
        KCHECK();
        for (int k = 0; k < 6; k++) if (outs[k]) HIPC(hipMemcpyAsync(outs[k], d_out + k * n, n * sizeof(double), hipMemcpyDeviceToHost, st));
        u32 flag = 0;
        HIPC(hipMemcpyAsync(&flag, stat + GEF_FLAG, sizeof flag, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        if (!(flag & NRM_CAND_SHORT)) { P.phen_ok[phen] = 1; return GEV_OK; }
    }
    P.phen_ok[phen] = 0;       // the short attempts have written the kept phenotype column: gev_compute_selection must not read it
    return fail(GEV_EDEVICE, "normal_stream: acceptance far below pi/4");
}

// Raw A/D totals of the current generation from the host: a locus-split population's contexts each hold partial sums; after the
// all-reduce (geneevolve_amd/distributed.py:compute_ad_locus_split) every context is given the totals, and
// gev_scale_ad_compute_gef then works as on an unsplit context.
int gev_set_ad(gev_ctx* c, int pop, const double* additive, const double* dominance)
{
    GEVC(check_idx(c, pop, 0));
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "set_ad: population %d has no current generation", pop);
    if (!additive || !dominance) return fail(GEV_EINVAL, "set_ad: null array");
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t nd = P.n_people * (size_t)c->nphen;
    GEVC(c->d_add.ensure(nd, st)); GEVC(c->d_dom.ensure(nd, st));
    HIPC(hipMemcpyAsync(c->d_add.p, additive, nd * sizeof(double), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(c->d_dom.p, dominance, nd * sizeof(double), hipMemcpyHostToDevice, st));
    HIPC(hipStreamSynchronize(st));
    c->ad_host_set_pop = pop;
    return GEV_OK;
}
// ---- Simulation::ras_compute_mating_value_selection_value + ras_selection_func (src/Simulation.cpp:3300-3342, :3386-3428) ----
// from the phenotypes gev_scale_ad_compute_gef left in the population, into its [3][n] value buffer; generation 0 also reduces the
// mean and variance of sv on the device.  Nothing waits unless an output is asked for.
int gev_compute_selection(gev_ctx* c, int pop, const gev_selection_params* par, double* mating_value, double* selection_value, double* selection_value_func)
{
    GEVC(check_idx(c, pop, 0));
    if (c->pend.active) return fail(GEV_ESTATE, "compute_selection: a generation is pending: call gev_generation_end / gev_reproduce_end first");
    if (!par || !par->omega || !par->lambda) return fail(GEV_EINVAL, "compute_selection: null parameters / omega / lambda");
    if (par->func < GEV_SEL_NONE || par->func > GEV_SEL_THR) return fail(GEV_EINVAL, "compute_selection: unknown selection function %d", par->func);
    if (par->gen_num < 0) return fail(GEV_EINVAL, "compute_selection: gen_num %d", par->gen_num);
    if (c->nphen > GEV_SEL_MAX_PHEN) return fail(GEV_EUNSUPPORTED, "compute_selection: more than %d phenotypes", GEV_SEL_MAX_PHEN);
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "compute_selection: population %d has no current generation", pop);
    for (int p = 0; p < c->nphen; p++)
        if (!P.phen_ok[p]) return fail(GEV_ESTATE, "compute_selection: phenotype %d of population %d's current generation has not been through gev_scale_ad_compute_gef", p, pop);
    const bool gen0 = par->gen_num == 0;
    if (!gen0 && !P.sv0_ok) return fail(GEV_ESTATE, "compute_selection: population %d has no generation-0 selection statistics (gen_num 0 first, or gev_set_selection_gen0)", pop);
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    SelArgs a{};
    a.nphen = c->nphen; a.func = par->func; a.gen_num = par->gen_num; a.par1 = par->par1; a.par2 = par->par2;
    for (int p = 0; p < c->nphen; p++) { a.omega[p] = par->omega[p]; a.lambda[p] = par->lambda[p]; a.shift[p] = par->phen_shift ? par->phen_shift[p] : 0.0; }
    const size_t n = P.n_people;
    Dev<double>& V = P.d_sel[P.sbuf];
    GEVC(V.ensure(3 * n, st));
    GEVC(P.d_sv0.ensure(2, st, /*keep=*/true));
    double *mv = V, *sv = mv + n, *svf = mv + 2 * n, *sv0 = P.d_sv0;
    const unsigned nbk = (unsigned)ceil_div(n, 256);
    hipLaunchKernelGGL(k_sel_values, dim3(nbk), dim3(256), 0, st, P.d_phen[P.sbuf], n, a, (const double*)sv0, gen0 ? 0 : 1, mv, sv, svf);
    if (gen0) {                                             // _gen0_SV_mean / _gen0_SV_var (:3326-3330), kept on the device
        GEVC(ph_var(c, sv, 1, 1, n, 1, sv0));
        hipLaunchKernelGGL(k_sel_finish, dim3(nbk), dim3(256), 0, st, n, a, (const double*)sv0, sv, svf);
    }
    KCHECK();
    if (gen0) P.sv0_ok = true;
    P.sel_ok = true;
    double* outs[3] = {mating_value, selection_value, selection_value_func};
    bool any = false;
    for (int k = 0; k < 3; k++) if (outs[k]) { HIPC(hipMemcpyAsync(outs[k], mv + k * n, n * sizeof(double), hipMemcpyDeviceToHost, st)); any = true; }
    if (any) HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
int gev_download_selection(gev_ctx* c, int pop, double* mating_value, double* selection_value, double* selection_value_func)
{
    GEVC(check_selection(c, pop, "download_selection"));
    PopState& P = c->pop[pop];
    HIPC(hipSetDevice(c->device));
    const size_t n = P.n_people;
    double* outs[3] = {mating_value, selection_value, selection_value_func};
    for (int k = 0; k < 3; k++) if (outs[k]) HIPC(hipMemcpyAsync(outs[k], P.d_sel[P.sbuf] + k * n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return GEV_OK;
}
int gev_get_selection_gen0(gev_ctx* c, int pop, double* mean, double* var)
{
    GEVC(check_idx(c, pop, 0));
    if (c->pend.active) return fail(GEV_ESTATE, "get_selection_gen0: a generation is pending");
    PopState& P = c->pop[pop];
    if (!P.sv0_ok) return fail(GEV_ESTATE, "get_selection_gen0: population %d has no generation-0 selection statistics", pop);
    HIPC(hipSetDevice(c->device));
    double h[2] = {0, 0};
    HIPC(hipMemcpyAsync(h, P.d_sv0.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if (mean) *mean = h[0];
    if (var) *var = h[1];
    return GEV_OK;
}
int gev_set_selection_gen0(gev_ctx* c, int pop, double mean, double var)
{
    GEVC(check_idx(c, pop, 0));
    if (c->pend.active) return fail(GEV_ESTATE, "set_selection_gen0: a generation is pending");
    PopState& P = c->pop[pop];
    HIPC(hipSetDevice(c->device));
    GEVC(P.d_sv0.ensure(2, c->stream));
    hipLaunchKernelGGL(k_sel_set_gen0, dim3(1), dim3(64), 0, c->stream, P.d_sv0, mean, var);
    KCHECK();
    P.sv0_ok = true;
    return GEV_OK;
}
int gev_get_cv_freq(gev_ctx* c, int pop, int phen, int chr, double* frq, size_t C)
{
    GEVC(check_idx(c, pop, chr, phen));
    GEVC(check_active(c, chr, "get_cv_freq"));
    CvStatic& V = c->pop[pop].cv[phen][chr];
    if (!V.frq_valid) return fail(GEV_ESTATE, "get_cv_freq: call gev_compute_ad first");
    if (C != V.C || !frq) return fail(GEV_EINVAL, "get_cv_freq: C=%zu, expected %u", C, V.C);
    HIPC(hipSetDevice(c->device));
    HIPC(hipMemcpyAsync(frq, V.d_frq.p, C * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return GEV_OK;
}

// ---- Simulation::ras_do_migration (row movement part) -------------------------------------
struct Seg { int src_pop; std::vector<u32> people; };     // individuals (positions in src_pop's current generation)
// The gather plan of one gev_migrate / materialize_order: for every destination the individuals of its non-empty segments, in segment
// order, and the haplotype rows 2p, 2p + 1 made from them -- uploaded ONCE into c->d_map, which nothing refills before the call's last
// gather has been enqueued ("One gather plan").  Segment g of a destination fills its individuals [g.i0, g.i0 + g.m).
struct PlanSeg { int src_pop; size_t i0, m; const u32* people; const u32* rows; };       // device: m individuals, 2m haplotype rows
struct GatherPlan { std::vector<std::vector<PlanSeg>> segs; std::vector<size_t> n_new; };  // [destination]
static int upload_plan(gev_ctx* c, const std::vector<std::vector<Seg>>& plan, GatherPlan& gp)
{
    gp.segs.assign(plan.size(), {}); gp.n_new.assign(plan.size(), 0);
    std::vector<u32> up;                                // [people | rows]
    for (const auto& segs : plan) for (const Seg& sg : segs) up.insert(up.end(), sg.people.begin(), sg.people.end());
    const size_t total = up.size();
    up.resize(3 * total);
    for (size_t j = 0; j < total; j++) { up[total + 2 * j] = 2 * up[j]; up[total + 2 * j + 1] = 2 * up[j] + 1; }
    GEVC(h2d(c, c->d_map, up.data(), up.size() * sizeof(u32)));
    const u32* d_people = c->d_map.as<u32>(); const u32* d_rows = d_people + total;
    size_t at = 0;
    for (size_t d = 0; d < plan.size(); d++) for (const Seg& sg : plan[d]) {
        const size_t m = sg.people.size();
        if (m) gp.segs[d].push_back(PlanSeg{sg.src_pop, gp.n_new[d], m, d_people + at, d_rows + 2 * at});
        gp.n_new[d] += m; at += m;
    }
    return GEV_OK;
}
extern "C++" {      // (templates cannot have the C linkage of the block this file's functions sit in)
// the one walk over a destination's segments: f(source population, segment)
template <class F>
static int for_segments(gev_ctx* c, const GatherPlan& gp, int dst, F f)
{
    for (const PlanSeg& g : gp.segs[dst]) GEVC(f(c->pop[g.src_pop], g));
    return GEV_OK;
}
// a value that follows the individuals stays valid where every population that contributes individuals had it
template <class Has>
static bool every_source(gev_ctx* c, const GatherPlan& gp, int dst, Has has)
{
    bool ok = true;
    for (const PlanSeg& g : gp.segs[dst]) ok = ok && has(c->pop[g.src_pop]);
    return ok;
}
}   // extern "C++"
// 8-byte planes (doubles, ids) of a segment's individuals: dst is the destination's plane 0 at the segment's i0
static int gather_planes(gev_ctx* c, unsigned planes, void* dst, size_t dstride, const void* src, size_t sstride, const PlanSeg& g)
{
    hipLaunchKernelGGL(k_gather_planes64, dim3((unsigned)ceil_div(g.m, 256), planes), dim3(256), 0, c->stream, (u64*)dst, dstride, (const u64*)src, sstride, g.people, g.m);
    KCHECK();
    return GEV_OK;
}
// The lists of the rows `rows` selects from the current generation of (P, k): from the CSR form where it is there (the cheaper one to
// read; always, behind ensure_csr), else from the pieces -- the only place that launches either pair of kernels for selected rows.
// Lengths: mcnt[n_rows], and pcnt[n_rows] with gev_set_track_intervals
static int selected_lists_count(gev_ctx* c, PopState& P, int k, const u32* rows, size_t n_rows, u32* mcnt, u32* pcnt)
{
    ChrState& cs = P.st[k];
    const bool track = c->track_intervals, pieces = !cs.csr_valid;
    if (pieces)
        hipLaunchKernelGGL(k_lp_count, dim3((unsigned)ceil_div(n_rows * LP_MAXSEG, 256)), dim3(256), 0, c->stream, track ? cs.lp.ptab[P.cur] : (const uint2*)nullptr,
                           cs.lp.mtab[P.cur], cs.lp.nseg, rows, n_rows, track ? pcnt : (u32*)nullptr, mcnt);
    else for (int pass = 0; pass < (track ? 2 : 1); pass++)
        hipLaunchKernelGGL(k_csr_gather_count, dim3((unsigned)ceil_div(n_rows, 256)), dim3(256), 0, c->stream, pass == 0 ? cs.moff[P.cur] : cs.poff[P.cur],
                           rows, n_rows, pass == 0 ? mcnt : pcnt);
    KCHECK();
    return GEV_OK;
}
// the lists themselves: row r of the selection goes behind mpos[moff[r]] / parts[poff[r]] (moff, poff: the caller's scans of the lengths)
static int selected_lists_fill(gev_ctx* c, PopState& P, int k, const u32* rows, size_t n_rows, const u32* moff, u64* mpos, const u32* poff, gev_part* parts)
{
    ChrState& cs = P.st[k];
    const bool track = c->track_intervals, pieces = !cs.csr_valid;
    const unsigned blocks = (unsigned)ceil_div(n_rows, 256);
    if (pieces)
        hipLaunchKernelGGL(k_lp_fill, dim3((unsigned)ceil_div(n_rows * LP_MAXSEG, 256)), dim3(256), 0, c->stream, track ? cs.lp.ptab[P.cur] : (const uint2*)nullptr,
                           cs.lp.mtab[P.cur], cs.lp.parena, cs.lp.marena, cs.lp.nseg, rows, n_rows, (u64)P.cs[k].rbp.back(), poff, parts, moff, mpos);
    else {
        hipLaunchKernelGGL((k_csr_gather_fill<u64>), dim3(blocks), dim3(256), 0, c->stream, cs.moff[P.cur], cs.mpos[P.cur], rows, n_rows, moff, mpos);
        if (track) hipLaunchKernelGGL((k_csr_gather_fill<gev_part>), dim3(blocks), dim3(256), 0, c->stream, cs.poff[P.cur], cs.parts[P.cur], rows, n_rows, poff, parts);
    }
    KCHECK();
    return GEV_OK;
}
// the logical positions of P name other rows than they did: couples left on the device and the cached A/D are void
static void positions_changed(gev_ctx* c, PopState& P) { P.layout_epoch++; c->ad_cached_pop = c->ad_host_set_pop = -1; }
// P lives in the buffers a gather wrote: n individuals in dense order (gev_migrate, materialize_order)
static void flip_to_gathered(gev_ctx* c, PopState& P, size_t n)
{
    P.cur ^= 1; P.pcur = (P.pcur + 1) % 3; P.n_people = P.n_phys = n; P.logical.clear();
    positions_changed(c, P);
}
// individuals left or joined by position (gev_remove_rows, gev_import_rows): the per-individual values did not follow them
static void membership_changed(gev_ctx* c, PopState& P)
{
    P.n_people = P.logical.size(); P.drop_selection(); P.ids_ok = false;
    positions_changed(c, P);
}
// rebuild population `dst` in its alternate buffers from its segments of the CURRENT buffers (in CSR form, capacity there); caller flips
static int gather_population(gev_ctx* c, int dst, const GatherPlan& gp)
{
    PopState& D = c->pop[dst];
    hipStream_t st = c->stream;
    const int alt = D.cur ^ 1;
    const size_t rows_new = 2 * gp.n_new[dst];
    const bool track = c->track_intervals;
    GEVC(c->d_cnt.ensure(2 * (rows_new + 1), st));
    u32* mcnt = c->d_cnt; u32* pcnt = mcnt + rows_new + 1;
    for (int k = 0; k < c->nchr; k++) {
        if (!c->chr_active[k]) continue;                // held by another context of a locus-split population
        ChrStatic& S = D.cs[k]; ChrState& ds = D.st[k];
        u32* moff = ds.moff[alt]; u32* poff = ds.poff[alt];
        GEVC(for_segments(c, gp, dst, [&](PopState& Sp, const PlanSeg& g) -> int { return selected_lists_count(c, Sp, k, g.rows, 2 * g.m, mcnt + 2 * g.i0, pcnt + 2 * g.i0); }));
        u32 tot_m = 0, tot_p = 0;                       // (the totals size the destination's list buffers: these syncs stay)
        GEVC(scan_u32(c, mcnt, rows_new, moff, &tot_m));
        if (track) GEVC(scan_u32(c, pcnt, rows_new, poff, &tot_p));
        GEVC(ds.mpos[alt].ensure(std::max<size_t>(tot_m, 2), st, false, 1.25)); ds.mut_total[alt] = tot_m;
        if (track) { GEVC(ds.parts[alt].ensure(std::max<size_t>(tot_p, 1), st, false, 1.25)); ds.parts_total[alt] = tot_p; }
        GEVC(for_segments(c, gp, dst, [&](PopState& Sp, const PlanSeg& g) -> int {
            return selected_lists_fill(c, Sp, k, g.rows, 2 * g.m, moff + 2 * g.i0, ds.mpos[alt], poff + 2 * g.i0, ds.parts[alt]);
        }));
        // genotype rows: fresh pool rows of the destination, filled from the sources' pools
        PoolWork dpw{};
        if (c->dense) {
            pool_new_stamp(ds);
            dpw = pool_work(c, D, k, (D.pcur + 1) % 3);
            GEVC(pool_free_list(dpw, 2 * D.n_phys, st));
            GEVC(pool_take(dpw, 0, rows_new, st));
            ds.pool_list_valid = false;                      // (the next generation builds its own list: the host's picture of this one is gone)
        }
        GEVC(for_segments(c, gp, dst, [&](PopState& Sp, const PlanSeg& g) -> int {
            const u32 chunks = (u32)(S.stride / 16);
            if (c->dense)
                hipLaunchKernelGGL(k_copy_rows16, dim3((unsigned)ceil_div(2 * g.m * chunks, 256)), dim3(256), 0, st,
                                   pool_rows(D, k, dpw.phys_alt + 2 * g.i0 * S.nseg), pool_rows(Sp, k, Sp.st[k].phys[Sp.pcur]), g.rows, (size_t)0, 2 * g.m, chunks);
            for (int p = 0; p < c->nphen; p++) {
                CvStatic& V = D.cv[p][k];
                const u32 cch = V.stride_w32 / 4;
                hipLaunchKernelGGL(k_gather_rows16, dim3((unsigned)ceil_div(2 * g.m * cch, 256)), dim3(256), 0, st,
                                   (uint4*)(D.cvp[p][k][alt] + 2 * g.i0 * V.stride_w32), (size_t)cch,
                                   (const uint4*)Sp.cvp[p][k][Sp.cur].p, (size_t)Sp.cv[p][k].stride_w32 / 4, g.rows, 2 * g.m, cch);
                V.frq_valid = false;
            }
            KCHECK();
            return GEV_OK;
        }));
    }
    // Human::sex follows the individuals (what gev_random_mate reads)
    GEVC(for_segments(c, gp, dst, [&](PopState& Sp, const PlanSeg& g) -> int {
        hipLaunchKernelGGL(k_gather_u8, dim3((unsigned)ceil_div(g.m, 256)), dim3(256), 0, st, D.d_sex[alt] + g.i0, Sp.d_sex[Sp.cur], g.people, 0u, g.m);
        KCHECK();
        return GEV_OK;
    }));
    for (int k = 0; k < c->nchr; k++) { D.st[k].csr_valid = true; D.st[k].lp.valid = false; }     // (the caller flips to the buffers written here: CSR form, no pieces yet)
    return GEV_OK;
}
// bring the current generation back to dense logical order (no-op unless rows were removed/imported)
static int materialize_order(gev_ctx* c, int pop)
{
    PopState& P = c->pop[pop];
    if (P.logical.empty()) return GEV_OK;
    GEVC(gev_sync(c));
    GEVC(ensure_csr(c, pop));                               // whole lists are read
    std::vector<std::vector<Seg>> plan(c->n_pop);
    plan[pop].push_back(Seg{pop, P.logical});
    GatherPlan gp;
    GEVC(upload_plan(c, plan, gp));
    GEVC(gather_population(c, pop, gp));
    if (P.ids_ok) {                                         // the pedigree ids are kept by physical row: they move with the rows
        const int nb = P.ibuf ^ 1;
        GEVC(P.d_ids[nb].ensure(PED_FIELDS * P.n_people, c->stream));
        GEVC(for_segments(c, gp, pop, [&](PopState& S, const PlanSeg& g) -> int {
            return gather_planes(c, PED_FIELDS, P.d_ids[nb] + g.i0, P.n_people, S.d_ids[S.ibuf].p, S.ids_stride[S.ibuf], g);
        }));
        P.ids_stride[nb] = P.n_people; P.ibuf = nb;
    }
    HIPC(hipStreamSynchronize(c->stream));
    P.cs_ok = false; P.comp_ok = false;
    flip_to_gathered(c, P, P.n_people);
    return GEV_OK;
}
static int check_not_pending(gev_ctx* c)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first");
    return GEV_OK;
}
// The phenotypes and Human::mating_value / selection_value / selection_value_func follow the individuals (the reference computes the
// values, src/Simulation.cpp:1988, before ras_do_migration, :1998): gathered into the other buffers of every destination, valid where
// every population that contributes individuals had them.  Called before the populations' sizes change.
static int migrate_selection(gev_ctx* c, const GatherPlan& gp)
{
    hipStream_t st = c->stream;
    const u32 nph = (u32)c->nphen;
    std::vector<uint8_t> phen_ok(c->n_pop), sel_ok(c->n_pop);
    for (int d = 0; d < c->n_pop; d++) {
        PopState& D = c->pop[d];
        const size_t n = gp.n_new[d];
        const int nb = D.sbuf ^ 1;
        phen_ok[d] = every_source(c, gp, d, [&](const PopState& S) { return std::all_of(S.phen_ok.begin(), S.phen_ok.end(), [](uint8_t v) { return v != 0; }); });
        sel_ok[d] = every_source(c, gp, d, [](const PopState& S) { return S.sel_ok; });
        if (phen_ok[d]) {                               // interleaved [n][nphen]
            GEVC(D.d_phen[nb].ensure(n * nph, st));
            GEVC(for_segments(c, gp, d, [&](PopState& S, const PlanSeg& g) -> int {
                hipLaunchKernelGGL(k_gather_f64, dim3((unsigned)ceil_div(g.m * nph, 256)), dim3(256), 0, st, D.d_phen[nb] + g.i0 * nph,
                                   S.d_phen[S.sbuf], g.people, g.m, nph);
                KCHECK();
                return GEV_OK;
            }));
        }
        if (sel_ok[d]) {                                // [3][n]: mating_value, selection_value, selection_value_func
            GEVC(D.d_sel[nb].ensure(3 * n, st));
            GEVC(for_segments(c, gp, d, [&](PopState& S, const PlanSeg& g) -> int { return gather_planes(c, 3, D.d_sel[nb] + g.i0, n, S.d_sel[S.sbuf].p, S.n_people, g); }));
        }
    }
    for (int d = 0; d < c->n_pop; d++) {
        PopState& D = c->pop[d];
        D.sbuf ^= 1; std::fill(D.phen_ok.begin(), D.phen_ok.end(), phen_ok[d]); D.sel_ok = sel_ok[d];
    }
    return GEV_OK;
}
// The pedigree ids follow the individuals as the selection values do (gev_set_track_pedigree); kept where every population that
// contributes individuals had them.  Called behind materialize_order: positions are physical rows.
static int migrate_pedigree(gev_ctx* c, const GatherPlan& gp)
{
    if (!c->track_pedigree) return GEV_OK;
    hipStream_t st = c->stream;
    const unsigned planes = (unsigned)c->nphen * PH_COMP;     // the phenotype components (gev_generation_phenotypes), plane by plane
    std::vector<uint8_t> ids_ok(c->n_pop), comp_ok(c->n_pop);
    for (int d = 0; d < c->n_pop; d++) {
        PopState& D = c->pop[d];
        const size_t n = gp.n_new[d];
        ids_ok[d] = every_source(c, gp, d, [](const PopState& S) { return S.ids_ok; });
        comp_ok[d] = every_source(c, gp, d, [](const PopState& S) { return S.comp_ok; });
        if (ids_ok[d]) {
            const int nb = D.ibuf ^ 1;
            GEVC(D.d_ids[nb].ensure(PED_FIELDS * n, st));
            GEVC(for_segments(c, gp, d, [&](PopState& S, const PlanSeg& g) -> int { return gather_planes(c, PED_FIELDS, D.d_ids[nb] + g.i0, n, S.d_ids[S.ibuf].p, S.ids_stride[S.ibuf], g); }));
        }
        if (comp_ok[d]) {
            const int nb = D.cbuf ^ 1;
            GEVC(D.d_comp[nb].ensure((size_t)planes * n, st));
            GEVC(for_segments(c, gp, d, [&](PopState& S, const PlanSeg& g) -> int { return gather_planes(c, planes, D.d_comp[nb] + g.i0, n, S.d_comp[S.cbuf].p, S.n_people, g); }));
        }
    }
    for (int d = 0; d < c->n_pop; d++) {
        PopState& D = c->pop[d];
        if (ids_ok[d]) { D.ibuf ^= 1; D.ids_stride[D.ibuf] = gp.n_new[d]; }
        if (comp_ok[d]) D.cbuf ^= 1;
        D.ids_ok = ids_ok[d]; D.comp_ok = comp_ok[d];
        D.cs_ok = false;                                    // (the children's couple indices belong to the rows as they were published)
    }
    return GEV_OK;
}
int gev_migrate(gev_ctx* c, const gev_move* moves, size_t n_moves)
{
    GEVC(check_not_pending(c));
    if (n_moves && !moves) return fail(GEV_EINVAL, "migrate: null moves");
    HIPC(hipSetDevice(c->device));
    GEVC(gev_sync(c));
    for (int p = 0; p < c->n_pop; p++) if (c->pop[p].gen0) GEVC(materialize_order(c, p));
    if (c->n_pop > 1 && !c->multipop_ready) GEVC(check_multipop(c));
    std::vector<std::vector<uint8_t>> gone(c->n_pop);
    for (int p = 0; p < c->n_pop; p++) {
        if (!c->pop[p].gen0) return fail(GEV_ESTATE, "migrate: population %d has no current generation", p);
        gone[p].assign(c->pop[p].n_people, 0);
    }
    for (size_t i = 0; i < n_moves; i++) {
        const gev_move& m = moves[i];
        if (m.src_pop < 0 || m.src_pop >= c->n_pop || m.dst_pop < 0 || m.dst_pop >= c->n_pop || m.src_pop == m.dst_pop)
            return fail(GEV_EINVAL, "migrate: move %zu has bad population indices", i);
        if (m.src_pos >= c->pop[m.src_pop].n_people || gone[m.src_pop][m.src_pos]) return fail(GEV_EINVAL, "migrate: move %zu: position out of range or moved twice", i);
        gone[m.src_pop][m.src_pos] = 1;
    }
    std::vector<std::vector<Seg>> plan(c->n_pop);
    for (int p = 0; p < c->n_pop; p++) {
        Seg keep; keep.src_pop = p;
        for (size_t i = 0; i < c->pop[p].n_people; i++) if (!gone[p][i]) keep.people.push_back((u32)i);   // stayers keep their order (:960-966)
        plan[p].push_back(std::move(keep));
    }
    for (size_t i = 0; i < n_moves; i++) {                                                              // migrants appended in `moves` order (:971-981)
        const gev_move& m = moves[i];
        if (plan[m.dst_pop].back().src_pop != m.src_pop || plan[m.dst_pop].size() == 1) { Seg s; s.src_pop = m.src_pop; plan[m.dst_pop].push_back(std::move(s)); }
        plan[m.dst_pop].back().people.push_back((u32)m.src_pos);
    }
    std::vector<size_t> n_new(c->n_pop, 0);
    for (int p = 0; p < c->n_pop; p++) {
        for (auto& s : plan[p]) n_new[p] += s.people.size();
        if (n_new[p] == 0) return fail(GEV_EINVAL, "migrate: population %d would become empty", p);
    }
    // grow every destination first (capacity growth copies the current buffers), then gather
    for (int p = 0; p < c->n_pop; p++) GEVC(ensure_capacity(c, p, n_new[p]));
    for (int p = 0; p < c->n_pop; p++) GEVC(ensure_csr(c, p));          // whole lists of every population are read (before any flag of a destination changes)
    GatherPlan gp;
    GEVC(upload_plan(c, plan, gp));                                     // the call's only upload of a gather map (gp.n_new == n_new)
    for (int p = 0; p < c->n_pop; p++) GEVC(gather_population(c, p, gp));
    GEVC(migrate_selection(c, gp));
    GEVC(migrate_pedigree(c, gp));
    HIPC(hipStreamSynchronize(c->stream));                              // every gather has read its sources before a buffer is flipped
    for (int p = 0; p < c->n_pop; p++) flip_to_gathered(c, c->pop[p], gp.n_new[p]);
    return GEV_OK;
}
// ---- cross-GPU form of the migration step ---------------------------------------------------
// The packed record's format and layout: gev_migrant_record.h.  Export and import fill and read its sections by index.
static_assert(MigrantRecord::MUT_BYTES == sizeof(u64) && MigrantRecord::PART_BYTES == sizeof(gev_part), "list entries of the migrant record");
// the record of n individuals of P whose header is `counts` (borrowed: it outlives the record)
static MigrantRecord migrant_record(gev_ctx* c, PopState& P, size_t n, const std::vector<u32>& counts)
{
    const int nchr = c->nchr;
    std::vector<size_t> stride(nchr), cv_row_bytes((size_t)c->nphen * nchr);
    for (int k = 0; k < nchr; k++) stride[k] = P.cs[k].stride;
    for (int p = 0; p < c->nphen; p++) for (int k = 0; k < nchr; k++) cv_row_bytes[(size_t)p * nchr + k] = P.cv[p][k].stride_w32 * sizeof(u32);
    return migrant_record_layout(n, nchr, c->nphen, c->chr_active.data(), c->dense && c->migrant_rows, stride.data(), cv_row_bytes.data(), counts.data());
}
// per-row list lengths of the selected individuals (device counts, one small D2H per chromosome); c->d_map then holds their
// haplotype rows 2*individual, 2*individual+1
static int export_counts(gev_ctx* c, int pop, const uint64_t* positions, size_t n, std::vector<u32>& counts)
{
    PopState& P = c->pop[pop];
    const int nchr = c->nchr;
    std::vector<u32> map(2 * n);
    for (size_t i = 0; i < n; i++) {
        if (positions[i] >= P.n_people) return fail(GEV_EINVAL, "export: position %llu beyond the population (%zu people)", (unsigned long long)positions[i], P.n_people);
        const u32 ph = P.logical.empty() ? (u32)positions[i] : P.logical[positions[i]];
        map[2 * i] = 2 * ph; map[2 * i + 1] = 2 * ph + 1;
    }
    counts.assign(MigrantRecord::n_counts(n, nchr), 0);
    if (!n) return GEV_OK;
    GEVC(h2d(c, c->d_map, map.data(), map.size() * sizeof(u32)));
    GEVC(c->d_cnt.ensure(4 * n + 4, c->stream));
    std::vector<u32> tmp(4 * n);                          // [mutations | interval parts] of the 2n rows
    for (int k = 0; k < nchr; k++) {
        if (!c->chr_active[k]) continue;
        GEVC(selected_lists_count(c, P, k, c->d_map.as<u32>(), 2 * n, c->d_cnt, c->d_cnt + 2 * n));
        HIPC(hipMemcpyAsync(tmp.data(), c->d_cnt.p, (c->track_intervals ? 4 : 2) * n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < n; i++) for (int h = 0; h < 2; h++) for (int pass = 0; pass < 2; pass++)
            counts[MigrantRecord::count_index(i, nchr, k, h, pass)] = tmp[pass * 2 * n + 2 * i + h];
    }
    return GEV_OK;
}
int gev_export_size(gev_ctx* c, int pop, const uint64_t* positions, size_t n, size_t* bytes)
{
    GEVC(check_idx(c, pop, 0));
    if (!bytes || (n && !positions)) return fail(GEV_EINVAL, "export_size: null argument");
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "export_size: population %d has no current generation", pop);
    HIPC(hipSetDevice(c->device));
    std::vector<u32> counts;
    GEVC(export_counts(c, pop, positions, n, counts));
    *bytes = migrant_record(c, P, n, counts).total;
    return GEV_OK;
}
int gev_export_rows(gev_ctx* c, int pop, const uint64_t* positions, size_t n, void* device_buf, size_t bytes)
{
    GEVC(check_idx(c, pop, 0));
    if (n && (!positions || !device_buf)) return fail(GEV_EINVAL, "export_rows: null argument");
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "export_rows: population %d has no current generation", pop);
    HIPC(hipSetDevice(c->device));
    GEVC(gev_sync(c));
    std::vector<u32> counts;
    GEVC(export_counts(c, pop, positions, n, counts));
    const MigrantRecord rec = migrant_record(c, P, n, counts);
    if (bytes < rec.total) return fail(GEV_EINVAL, "export_rows: buffer of %zu bytes, %zu needed", bytes, rec.total);
    if (!n) return GEV_OK;
    hipStream_t st = c->stream;
    uint8_t* out = (uint8_t*)device_buf;
    const int nchr = c->nchr;
    const u32* d_rows = c->d_map.as<u32>();               // haplotype rows 2*individual, 2*individual+1 (export_counts)
    HIPC(hipMemcpyAsync(out + rec.counts_at, counts.data(), counts.size() * sizeof(u32), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gather_u8, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, out + rec.sex_at, P.d_sex[P.cur], d_rows, 1u, n);
    GEVC(c->d_cnt.ensure((2 * n + 1) * 4, st));
    u32* mcnt = c->d_cnt; u32* moff = mcnt + (2 * n + 1); u32* pcnt = moff + (2 * n + 1); u32* poff = pcnt + (2 * n + 1);
    for (int k = 0; k < nchr; k++) {
        if (!c->chr_active[k]) continue;
        ChrStatic& S = P.cs[k]; ChrState& cs = P.st[k];
        const u32 chunks = (u32)(S.stride / 16);
        if (c->dense && c->migrant_rows)
            hipLaunchKernelGGL(k_copy_rows16, dim3((unsigned)ceil_div(2 * n * chunks, 256)), dim3(256), 0, st, flat_rows(out + rec.planes_at(k), S.stride),
                               pool_rows(P, k, cs.phys[P.pcur]), d_rows, (size_t)0, 2 * n, chunks);
        // the records' lists, for the selected rows only, from whichever form the lists live in
        GEVC(selected_lists_count(c, P, k, d_rows, 2 * n, mcnt, pcnt));
        GEVC(scan_u32(c, mcnt, 2 * n, moff, nullptr));
        if (c->track_intervals) GEVC(scan_u32(c, pcnt, 2 * n, poff, nullptr));
        GEVC(selected_lists_fill(c, P, k, d_rows, 2 * n, moff, (u64*)(out + rec.muts_at(k)), poff, (gev_part*)(out + rec.parts_at(k))));
    }
    for (int p = 0; p < c->nphen; p++) for (int k = 0; k < nchr; k++) {
        if (!c->chr_active[k]) continue;
        const u32 cch = P.cv[p][k].stride_w32 / 4;
        hipLaunchKernelGGL(k_gather_rows16, dim3((unsigned)ceil_div(2 * n * cch, 256)), dim3(256), 0, st, (uint4*)(out + rec.cv_at(p, k)), (size_t)cch,
                           (const uint4*)P.cvp[p][k][P.cur].p, (size_t)cch, d_rows, 2 * n, cch);
    }
    KCHECK();
    HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
int gev_remove_rows(gev_ctx* c, int pop, const uint64_t* positions, size_t n)
{
    GEVC(check_idx(c, pop, 0));
    if (n && !positions) return fail(GEV_EINVAL, "remove_rows: null positions");
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "remove_rows: population %d has no current generation", pop);
    std::vector<uint8_t> gone(P.n_people, 0);
    for (size_t i = 0; i < n; i++) {
        if (positions[i] >= P.n_people || gone[positions[i]]) return fail(GEV_EINVAL, "remove_rows: position out of range or listed twice");
        gone[positions[i]] = 1;
    }
    if (n >= P.n_people) return fail(GEV_EINVAL, "remove_rows: population %d would become empty", pop);
    // no row moves: only the logical order changes; stayers keep their order (src/Simulation.cpp:960-966)
    std::vector<u32> keep; keep.reserve(P.n_people - n);
    for (size_t i = 0; i < P.n_people; i++) if (!gone[i]) keep.push_back(P.logical.empty() ? (u32)i : P.logical[i]);
    P.logical.swap(keep);
    membership_changed(c, P);
    return GEV_OK;
}
// ---- gev_import_rows: its steps, in the order the driver below issues them.  n immigrants become the physical rows r_old .. r_old + 2n
struct ImportTrace {                                                  // GEV_TRACE_HOST: where an import's time goes (serialises the steps)
    hipStream_t st; double t;
    void mark(const char* what)
    {
        if (g_trace_host) { (void)hipStreamSynchronize(st); const double now = host_ms(); fprintf(stderr, "[gev] import_rows %s %.3f ms\n", what, now - t); t = now; }
    }
};
// leaves: the record's header in `counts`, its layout in `rec`, size and state checked, the rebuild flag zeroed where rows are rebuilt
static int import_header(gev_ctx* c, PopState& P, const uint8_t* in, size_t bytes, size_t n, std::vector<u32>& counts, MigrantRecord& rec)
{
    hipStream_t st = c->stream;
    if (bytes < MigrantRecord::n_counts(n, c->nchr) * sizeof(u32)) return fail(GEV_EINVAL, "import_rows: buffer too small for its own header");
    counts.resize(MigrantRecord::n_counts(n, c->nchr));
    HIPC(hipMemcpyAsync(counts.data(), in, counts.size() * sizeof(u32), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    rec = migrant_record(c, P, n, counts);
    if (bytes < rec.total) return fail(GEV_EINVAL, "import_rows: buffer of %zu bytes, %zu expected from its header", bytes, rec.total);
    const bool rebuild = c->dense && !c->migrant_rows;
    if (rebuild && !c->track_intervals) return fail(GEV_ESTATE, "import_rows: migrants without genotype rows need the interval state (gev_set_track_intervals)");
    if (rebuild) { GEVC(c->d_flag.ensure(16, st)); HIPC(hipMemsetAsync(c->d_flag.p, 0, 4, st)); }
    if ((P.n_phys + n) * 2 >= 0xffffffffull) return fail(GEV_EINVAL, "import_rows: too many rows");
    return GEV_OK;
}
// leaves: pool units for the new rows of chromosome k in the current generation's table, `dst` naming those rows: from the free list the generations
// keep (its entries behind the cursor are named by no table, and nothing is in flight after gev_sync) while it lasts, else from a new one
static int import_units(gev_ctx* c, PopState& P, int k, size_t r_old, size_t n, ImportTrace& tr, RowRef& dst)
{
    ChrState& cs = P.st[k];
    const size_t need_units = 2 * n * P.cs[k].nseg;
    const bool reuse = cs.pool_list_valid && !cs.pool_force_rebuild && (size_t)cs.pool_cursor + need_units <= cs.pool_n_free;
    if (!reuse) pool_new_stamp(cs);
    const PoolWork pw = pool_work(c, P, k, P.pcur);                 // new slots of the CURRENT generation
    if (!reuse) GEVC(pool_free_list(pw, r_old, c->stream));
    tr.mark("free list");
    GEVC(pool_take(pw, r_old, 2 * n, c->stream));
    if (reuse) cs.pool_cursor += (u32)need_units; else cs.pool_list_valid = false;
    tr.mark("units");
    dst = pool_rows(P, k, pw.phys_alt + r_old * P.cs[k].nseg);
    return GEV_OK;
}
// leaves: the new rows of chromosome k copied from the record's [planes] section (enqueued)
static int import_rows_copied(gev_ctx* c, PopState& P, int k, const MigrantRecord& rec, const uint8_t* in, const RowRef& dst, size_t n)
{
    const u32 chunks = (u32)(P.cs[k].stride / 16);
    hipLaunchKernelGGL(k_copy_rows16, dim3((unsigned)ceil_div(2 * n * chunks, 256)), dim3(256), 0, c->stream, dst,
                       flat_rows((void*)(in + rec.planes_at(k)), P.cs[k].stride), (const u32*)nullptr, (size_t)0, 2 * n, chunks);
    KCHECK();
    return GEV_OK;
}
// leaves: the new rows of chromosome k rebuilt (enqueued; c->d_flag tells of a missing panel or hap_index): the migrants travelled as lists, their
// rows are the founder mosaic their ancestry intervals describe (:1198-1211), assembled from the founder panels of the parts' root populations
static int import_rows_rebuilt(gev_ctx* c, PopState& P, int k, const MigrantRecord& rec, const uint8_t* in, const RowRef& dst, size_t n)
{
    hipStream_t st = c->stream;
    const ChrStatic& S = P.cs[k];
    const u32 chunks = (u32)(S.stride / 16);
    const gev_part* parts = (const gev_part*)(in + rec.parts_at(k));
    const std::vector<u32> offp = rec.row_offsets(k, 1);
    std::vector<PanelRef> pr(c->n_pop);
    for (int q = 0; q < c->n_pop; q++) {
        const ChrStatic& F = c->pop[q].cs[k];
        pr[q] = PanelRef{F.panel.as<u32>(), (u64)(F.stride / 4), (F.panel_rows && F.L == S.L) ? (u64)F.panel_rows : 0ull};
    }
    // one upload: the rows' part offsets, then the panel table (8-byte aligned behind them)
    const size_t off_words = (offp.size() + 1) & ~(size_t)1;
    std::vector<u32> up(off_words + pr.size() * sizeof(PanelRef) / sizeof(u32), 0);
    memcpy(up.data(), offp.data(), offp.size() * sizeof(u32)); memcpy(up.data() + off_words, pr.data(), pr.size() * sizeof(PanelRef));
    GEVC(h2d(c, c->d_poff, up.data(), up.size()));
    const PanelRef* d_panels = (const PanelRef*)(c->d_poff + off_words);
    GEVC(c->d_prange.ensure(std::max<size_t>(offp[2 * n], 1), st));
    if (offp[2 * n]) hipLaunchKernelGGL(k_parts_locus_range, dim3((unsigned)ceil_div((size_t)offp[2 * n], 256)), dim3(256), 0, st, parts, (size_t)offp[2 * n],
                                        P.d_chrdev, k, c->d_prange);
    hipLaunchKernelGGL(k_rebuild_rows, dim3((unsigned)(2 * n), (unsigned)ceil_div(chunks, 4 * REBUILD_CPW)), dim3(256), 0, st, c->d_poff, parts,
                       c->d_prange, (u32)S.L, d_panels, c->n_pop, dst, chunks, c->d_flag.as<u32>());
    KCHECK();
    return GEV_OK;
}
// leaves: the new rows' lists of chromosome k appended as pieces of their own behind the arenas, their table rows written behind the
// existing ones, the arena fill counts taken (one host wait); nothing of the residents is touched
static int import_list_pieces(gev_ctx* c, PopState& P, int k, const MigrantRecord& rec, const uint8_t* in, size_t r_old, size_t n)
{
    hipStream_t st = c->stream;
    ChrState::LpState& lp = P.st[k].lp;
    const bool track = c->track_intervals;
    const std::vector<u32> offm = rec.row_offsets(k, 0), offp = rec.row_offsets(k, 1);
    GEVC(c->d_cnt.ensure((2 * n + 1) * 2, st));
    u32* d_offm = c->d_cnt; u32* d_offp = d_offm + (2 * n + 1);
    HIPC(hipMemcpyAsync(d_offm, offm.data(), (2 * n + 1) * sizeof(u32), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_offp, offp.data(), (2 * n + 1) * sizeof(u32), hipMemcpyHostToDevice, st));
    const size_t tab_entries = (r_old + 2 * n) * lp.nseg;
    if (track) GEVC(lp.ptab[P.cur].ensure(tab_entries, st, /*keep=*/true, 1.25));
    GEVC(lp.mtab[P.cur].ensure(tab_entries, st, /*keep=*/true, 1.25));
    const size_t need_p = track ? (size_t)lp.p_used + offp[2 * n] + 2 * n * lp.nseg : 0, need_m = (size_t)lp.m_used + offm[2 * n];
    if (need_p >= 0xfffffff0u || need_m >= 0xfffffff0u) return fail(GEV_EDEVICE, "import_rows: list arenas beyond 2^32 entries");
    if (track && need_p > lp.parena.capacity()) GEVC(lp.parena.ensure(need_p, st, true, 1.5));
    if (need_m > lp.marena.capacity()) GEVC(lp.marena.ensure(std::max<size_t>(need_m, 16), st, true, 1.5));
    HIPC(hipMemsetAsync(lp.ctr.p, 0, 4 * sizeof(u32), st));
    hipLaunchKernelGGL(k_lp_import, dim3((unsigned)ceil_div(2 * n * LP_MAXSEG, 256)), dim3(256), 0, st,
                       track ? d_offp : (const u32*)nullptr, track ? (const gev_part*)(in + rec.parts_at(k)) : (const gev_part*)nullptr, d_offm, (const u64*)(in + rec.muts_at(k)),
                       r_old, 2 * n, track ? lp.ptab[P.cur] : (uint2*)nullptr, lp.mtab[P.cur], lp.parena, lp.marena,
                       lp.p_used, lp.m_used, (u32)(lp.parena.capacity()), (u32)(lp.marena.capacity()), lp.nseg, lp.lgw, (u64)P.cs[k].rbp.front(),
                       lp.ctr, lp.ctr + 2);
    KCHECK();
    u32 h[4] = {0, 0, 0, 0};
    HIPC(hipMemcpyAsync(h, lp.ctr.p, sizeof h, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (h[2]) return fail(GEV_EDEVICE, "import_rows: list arena overflow (internal error)");
    lp.p_used += h[0]; lp.m_used += h[1];
    P.st[k].csr_valid = false;
    return GEV_OK;
}
// leaves: one kind of list (T: u64 mutations, gev_part intervals) of the new rows appended in CSR form: `off`, the rows' offsets from the old
// total on, at entries r_old .. r_old + 2n of doff (entry r_old already equals the old total), the elements behind `data`
extern "C++" template <class T> static int import_csr_list(gev_ctx* c, const std::vector<u32>& off, const T* src, size_t r_old, Dev<u32>& doff, Dev<T>& data, size_t& total, size_t min_elems)
{
    hipStream_t st = c->stream;
    const size_t add = off.back() - off[0];
    HIPC(hipMemcpyAsync(doff + r_old, off.data(), off.size() * sizeof(u32), hipMemcpyHostToDevice, st));
    HIPC(hipStreamSynchronize(st));
    GEVC(data.ensure(std::max<size_t>(total + add, min_elems), st, /*keep=*/true, 1.25));
    if (add) HIPC(hipMemcpyAsync(data + total, src, add * sizeof(T), hipMemcpyDeviceToDevice, st));
    total += add;
    return GEV_OK;
}
// leaves: the new rows' CV rows of every (phenotype, chromosome) behind the existing ones (enqueued), the allele frequencies stale
static int import_cv_rows(gev_ctx* c, PopState& P, const MigrantRecord& rec, const uint8_t* in, size_t r_old, size_t n)
{
    for (int p = 0; p < c->nphen; p++) for (int k = 0; k < c->nchr; k++) {
        if (!c->chr_active[k]) continue;
        CvStatic& V = P.cv[p][k];
        HIPC(hipMemcpyAsync(P.cvp[p][k][P.cur] + r_old * V.stride_w32, in + rec.cv_at(p, k), 2 * n * V.stride_w32 * sizeof(u32), hipMemcpyDeviceToDevice, c->stream));
        V.frq_valid = false;
    }
    return GEV_OK;
}
// leaves: everything enqueued done and the rebuild flag checked; the n new individuals behind the others in the logical order
static int import_finish(gev_ctx* c, PopState& P, size_t n_old, size_t n)
{
    u32 rb_flag = 0;
    if (c->dense && !c->migrant_rows) HIPC(hipMemcpyAsync(&rb_flag, c->d_flag.p, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if (rb_flag & 2u) return fail(GEV_ESTATE, "import_rows: an immigrant descends from a root population whose founder panel is not held here (gev_upload_founder_panel / gev_synth_founder_panel)");
    if (rb_flag & 1u) return fail(GEV_EINVAL, "import_rows: Error: p.hap_index is not in range");
    if (P.logical.empty()) { P.logical.resize(P.n_people); for (size_t i = 0; i < P.n_people; i++) P.logical[i] = (u32)i; }
    for (size_t i = 0; i < n; i++) P.logical.push_back((u32)(n_old + i));
    P.n_phys = n_old + n;
    membership_changed(c, P);
    return GEV_OK;
}
int gev_import_rows(gev_ctx* c, int pop, const void* device_buf, size_t bytes, size_t n)
{
    GEVC(check_idx(c, pop, 0));
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "import_rows: population %d has no current generation", pop);
    if (!n) return GEV_OK;
    if (!device_buf) return fail(GEV_EINVAL, "import_rows: null buffer");
    HIPC(hipSetDevice(c->device));
    GEVC(gev_sync(c));
    const uint8_t* in = (const uint8_t*)device_buf;
    ImportTrace tr{c->stream, host_ms()};
    std::vector<u32> counts; MigrantRecord rec;
    GEVC(import_header(c, P, in, bytes, n, counts, rec));
    const size_t n_old = P.n_phys, r_old = 2 * n_old;                  // physical append behind every existing row
    tr.mark("header");
    GEVC(ensure_capacity(c, pop, n_old + n));                           // keeps the current buffers' content
    tr.mark("capacity");
    HIPC(hipMemcpyAsync(P.d_sex[P.cur] + n_old, in + rec.sex_at, n, hipMemcpyDeviceToDevice, c->stream));
    for (int k = 0; k < c->nchr; k++) {
        if (!c->chr_active[k]) continue;
        ChrState& cs = P.st[k];
        if (c->dense) {
            RowRef dst{};
            GEVC(import_units(c, P, k, r_old, n, tr, dst));
            GEVC(c->migrant_rows ? import_rows_copied(c, P, k, rec, in, dst, n) : import_rows_rebuilt(c, P, k, rec, in, dst, n));
            tr.mark("rows");
        }
        if (cs.lp.valid) {
            GEVC(import_list_pieces(c, P, k, rec, in, r_old, n));
            tr.mark("list pieces");
        } else {
            GEVC(import_csr_list(c, rec.row_offsets(k, 0, (u32)cs.mut_total[P.cur]), (const u64*)(in + rec.muts_at(k)), r_old, cs.moff[P.cur], cs.mpos[P.cur], cs.mut_total[P.cur], 2));
            if (c->track_intervals)
                GEVC(import_csr_list(c, rec.row_offsets(k, 1, (u32)cs.parts_total[P.cur]), (const gev_part*)(in + rec.parts_at(k)), r_old, cs.poff[P.cur], cs.parts[P.cur], cs.parts_total[P.cur], 1));
        }
    }
    GEVC(import_cv_rows(c, P, rec, in, r_old, n));
    return import_finish(c, P, n_old, n);
}

// ---- output materialisation ---------------------------------------------------------------
// units (haplotype rows, individuals, SNPs) one staging pass of an output call takes: what fits the call's byte budget, at least 1;
// SNPs in multiples of 64, at least 64.  The only place that knows the test cap of gev_dbg_output_chunk
static size_t output_chunk(const gev_ctx* c, size_t budget_bytes, size_t bytes_per_unit, bool snps = false)
{
    size_t n = std::max<size_t>(budget_bytes / std::max<size_t>(bytes_per_unit, 1), 1);
    if (c->dbg_output_chunk) n = std::min(n, c->dbg_output_chunk);
    return snps ? std::max<size_t>(n, 64) & ~(size_t)63 : n;
}
// test hook: no staging pass of the following output calls takes more than max_units units (0: the byte budgets alone decide again)
int gev_dbg_output_chunk(gev_ctx* c, size_t max_units)
{
    GEVC(check_not_pending(c));
    c->dbg_output_chunk = max_units;
    return GEV_OK;
}
// what every output call on (pop, chr) begins with; planes: the call reads the resident genotype planes
static int output_begin(gev_ctx* c, int pop, int chr, const char* who, bool planes)
{
    GEVC(check_idx(c, pop, chr));
    if (planes) GEVC(check_dense(c, who));
    GEVC(check_active(c, chr, who));
    if (!c->pop[pop].gen0) return fail(GEV_ESTATE, "%s: population %d has no current generation", who, pop);
    HIPC(hipSetDevice(c->device));
    GEVC(materialize_order(c, pop));
    if (planes) GEVC(wait_planes(c));
    return GEV_OK;
}
static int check_range(const char* who, const char* noun, size_t begin, size_t n, size_t bound)
{
    if (begin + n > bound) return fail(GEV_EINVAL, "%s: %s [%zu,%zu) beyond the %zu there are", who, noun, begin, begin + n, bound);
    return GEV_OK;
}
// the caller's buffer of a request for n things: `have` of `need` (bytes, or words per row)
static int check_out(const char* who, const void* out, size_t n, size_t have, size_t need, const char* unit)
{
    if (n && (!out || have < need)) return fail(GEV_EINVAL, "%s: output buffer of %zu %s, %zu needed", who, have, unit, need);
    return GEV_OK;
}
// the haplotype-major rows of L SNPs in host memory that a gev_dbg_*_host form reads (needed: the request reads any)
static int check_host_rows(const char* who, const uint64_t* bits, size_t row_stride_words, size_t L, bool needed)
{
    if (needed && (!bits || row_stride_words < ceil_div(L, 64))) return fail(GEV_EINVAL, "%s: rows of %zu words, %zu needed", who, row_stride_words, ceil_div(L, 64));
    return GEV_OK;
}
// n_rows device rows of row_bytes bytes (pitch d_pitch) into the caller's rows of row_stride_words words, the pad behind each row
// zeroed; returns when they have arrived
static int copy_out_rows(gev_ctx* c, const void* d_rows, size_t d_pitch, size_t row_bytes, size_t n_rows, u64* bits, size_t row_stride_words)
{
    const size_t pitch = row_stride_words * 8;
    if (pitch > row_bytes) for (size_t r = 0; r < n_rows; r++) memset((uint8_t*)bits + r * pitch + row_bytes, 0, pitch - row_bytes);
    if (row_bytes) HIPC(hipMemcpy2DAsync(bits, pitch, d_rows, d_pitch, row_bytes, n_rows, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return GEV_OK;
}
// haplotype slots [slot0, slot0 + n) of the current generation, mutations applied, contiguous in c->d_stage (already large enough;
// ensure_csr has run: the mutation overlay reads whole lists)
static int stage_rows_mutated(gev_ctx* c, PopState& P, int chr, size_t slot0, size_t n)
{
    ChrStatic& S = P.cs[chr]; ChrState& cs = P.st[chr];
    const u32 chunks = (u32)(S.stride / 16);
    if (!n) return GEV_OK;
    hipLaunchKernelGGL(k_copy_rows16, dim3((unsigned)ceil_div(n * chunks, 256)), dim3(256), 0, c->stream, flat_rows(c->d_stage.p, S.stride),
                       pool_rows(P, chr, cs.phys[P.pcur]), (const u32*)nullptr, slot0, n, chunks);
    hipLaunchKernelGGL(k_snp_apply_mut, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, c->stream,
                       row_map(P, chr), c->d_stage.as<u32>(), S.stride / 4, slot0, n,
                       cs.moff[P.cur], cs.mpos[P.cur], S.d_pos, (u32)S.L);
    KCHECK();
    return GEV_OK;
}
// SNP-major bit matrix of SNPs [s0, s0+ns) of the current generation (mutations applied) into c->d_snpmajor
static int snp_major_device(gev_ctx* c, int pop, int chr, size_t s0, size_t ns, size_t& stride_w64)
{
    PopState& P = c->pop[pop]; ChrStatic& S = P.cs[chr]; ChrState& cs = P.st[chr];
    hipStream_t st = c->stream;
    GEVC(ensure_csr(c, pop));
    const size_t rows = 2 * P.n_people;
    stride_w64 = ceil_div(rows, 64);
    GEVC(c->d_snpmajor.ensure(std::max<size_t>(ns * stride_w64 * 8, 16), st));
    HIPC(hipMemsetAsync(c->d_snpmajor.p, 0, ns * stride_w64 * 8, st));
    const u32 n_words = (u32)(((s0 + ns - 1) >> 6) - (s0 >> 6) + 1);
    const u32 wpw = 16;                                              // 16 words = one 128-byte line of every row per wave
    const unsigned gy = (unsigned)ceil_div(ceil_div(n_words, wpw), 4);
    hipLaunchKernelGGL(k_transpose_tiles, dim3((unsigned)stride_w64, gy), dim3(256), 0, st, (const u64*)nullptr, row_map(P, chr), S.stride / 8, rows, (u32)S.L,
                       (u32)s0, (u32)ns, c->d_snpmajor.as<u64>(), stride_w64, wpw);
    hipLaunchKernelGGL(k_snpmajor_apply_mut, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, st, row_map(P, chr), rows,
                       cs.moff[P.cur], cs.mpos[P.cur], S.d_pos, (u32)S.L, (u32)s0, (u32)ns,
                       c->d_snpmajor.as<unsigned long long>(), stride_w64);
    KCHECK();
    return GEV_OK;
}
extern "C++" {      // (templates cannot have the C linkage of the block this file's functions sit in)
// `bytes` of text through c->d_text: launch() enqueues the kernel that writes them there; returns when they have arrived in dst
template <class Launch>
static int copy_out_text(gev_ctx* c, size_t bytes, void* dst, Launch launch)
{
    GEVC(c->d_text.ensure(bytes, c->stream));
    launch();
    KCHECK();
    HIPC(hipMemcpyAsync(dst, c->d_text.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return GEV_OK;
}
// SNPs [snp_begin, +n_snps) through c->d_snpmajor in chunks that keep the staging buffers <= ~256 MB at bytes_per_snp each:
// emit(s, ns, stride) delivers SNPs [snp_begin + s, +ns) (device rows of `stride` words) and returns when the host has them
template <class Emit>
static int snp_major_chunks(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, size_t bytes_per_snp, Emit emit)
{
    const size_t chunk = output_chunk(c, 256u << 20, bytes_per_snp, true);
    for (size_t s = 0; s < n_snps; s += chunk) {
        const size_t ns = std::min(chunk, n_snps - s); size_t stride;
        GEVC(snp_major_device(c, pop, chr, snp_begin + s, ns, stride));
        GEVC(emit(s, ns, stride));
    }
    return GEV_OK;
}
// the formatted ones, after output_begin: `line` bytes per SNP into out; launch(ns, stride) enqueues the kernel that formats ns SNPs
// of c->d_snpmajor into c->d_text
template <class Launch>
static int format_snp_major(gev_ctx* c, int pop, int chr, const char* who, size_t snp_begin, size_t n_snps, size_t line, size_t bytes_per_snp,
                            void* out, size_t out_bytes, Launch launch)
{
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, c->pop[pop].cs[chr].L));
    GEVC(check_out(who, out, n_snps, out_bytes, n_snps * line, "bytes"));
    return snp_major_chunks(c, pop, chr, snp_begin, n_snps, bytes_per_snp, [&](size_t s, size_t ns, size_t stride) -> int {
        return copy_out_text(c, ns * line, (char*)out + s * line, [&] { launch(ns, stride); });
    });
}
// individuals [ind_begin, +n_ind) as hap-major rows (mutations applied) through c->d_stage in chunks of <= ~256 MB of output at
// bytes_per_ind each: emit(i, n) delivers individuals [ind_begin + i, +n) from the staged rows and returns when the host has them
template <class Emit>
static int ind_major_chunks(gev_ctx* c, int pop, int chr, size_t ind_begin, size_t n_ind, size_t bytes_per_ind, Emit emit)
{
    PopState& P = c->pop[pop];
    const size_t chunk = output_chunk(c, 256u << 20, bytes_per_ind);
    for (size_t i = 0; i < n_ind; i += chunk) {
        const size_t n = std::min(chunk, n_ind - i);
        GEVC(c->d_stage.ensure(std::max<size_t>(2 * n * P.cs[chr].stride, 16), c->stream));
        GEVC(ensure_csr(c, pop));
        GEVC(stage_rows_mutated(c, P, chr, 2 * (ind_begin + i), 2 * n));
        GEVC(emit(i, n));
    }
    return GEV_OK;
}
// a CSR list of the current generation to the host: *n = its length, hap_offsets[2 * n_people + 1] and the elements where asked for
template <class T>
static int download_list(gev_ctx* c, int pop, const char* who, const Dev<u32>& d_off, const Dev<T>& d_val, T* out, u64* hap_offsets, size_t* n)
{
    if (!n) return fail(GEV_EINVAL, "%s: the list length has nowhere to go (null)", who);
    const size_t rows = 2 * c->pop[pop].n_people;
    std::vector<u32> off(rows + 1);
    HIPC(hipMemcpyAsync(off.data(), d_off.p, (rows + 1) * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    *n = off[rows];
    if (hap_offsets) for (size_t r = 0; r <= rows; r++) hap_offsets[r] = off[r];
    if (out && off[rows]) {
        HIPC(hipMemcpyAsync(out, d_val.p, (size_t)off[rows] * sizeof(T), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    return GEV_OK;
}
// The record lists (gev_ibd_segments, gev_roh_segments) in three steps over c->list (cnt, off, tot).  What the device
// and the host forms refuse of a list's own arguments:
static int list_args(const char* who, const void* out, size_t capacity, const uint64_t* n_total)
{
    if (!n_total) return fail(GEV_EINVAL, "%s: n_total is null", who);
    if (!out && capacity) return fail(GEV_EINVAL, "%s: a null output of capacity %zu", who, capacity);
    return GEV_OK;
}
// the sum of the n counts at d_cnt in 64 bits, in host memory when this returns
static int count_total(gev_ctx* c, const u32* d_cnt, size_t n, u64* total)
{
    hipStream_t st = c->stream;
    GEVC(c->list.tot.ensure(1, st));
    HIPC(hipMemsetAsync(c->list.tot.p, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_total_u32, dim3((unsigned)std::min<size_t>(ceil_div(n, 1024), 1024)), dim3(256), 0, st, d_cnt, n, c->list.tot.p);
    KCHECK();
    unsigned long long t = 0;
    HIPC(hipMemcpyAsync(&t, c->list.tot.p, sizeof t, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    *total = t;
    return GEV_OK;
}
// the `total` records (< 2^32: no offset wraps) of the n items counted in c->list.cnt into out (host): the counts are scanned into
// c->list.off, launch() enqueues the kernel that fills d_rec (already large enough) from those offsets; returns when they have arrived
template <class T, class Launch>
static int fill_list(gev_ctx* c, size_t n, u64 total, const Dev<T>& d_rec, T* out, Launch launch)
{
    hipStream_t st = c->stream;
    GEVC(c->list.off.ensure(n + 1, st));
    GEVC(scan_u32_on(st, c->d_sums, c->list.cnt.p, n, c->list.off.p));
    GEVC(launch());
    HIPC(hipMemcpyAsync(out, d_rec.p, (size_t)total * sizeof(T), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
// An optional result vector of a call: `count` elements of `el` bytes, wanted where host is not null, made at dev (the calls pack theirs
// into one device buffer, 8-byte elements first: every part begins on a multiple of its element)
struct OptOut { void* host; size_t el, count; const void* dev = nullptr; };
template <size_t N>
static void zero_outs(const OptOut (&outs)[N])
{
    for (const OptOut& o : outs) if (o.host) memset(o.host, 0, o.count * o.el);
}
// the wanted ones to the host, in the table's order; returns when they have arrived
template <size_t N>
static int copy_back_outs(gev_ctx* c, const OptOut (&outs)[N])
{
    for (const OptOut& o : outs) if (o.host) HIPC(hipMemcpyAsync(o.host, o.dev, o.count * o.el, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return GEV_OK;
}
// a sub-block's results dev ([na][nb] elements of el bytes) into the caller's matrix host (rows of n_b) at (ia, ib), behind the stream's work
static int copy_out_block(gev_ctx* c, void* host, size_t el, size_t n_b, size_t ia, size_t ib, size_t na, size_t nb, const void* dev)
{
    char* dst = (char*)host + (ia * n_b + ib) * el;
    if (nb == n_b) HIPC(hipMemcpyAsync(dst, dev, na * nb * el, hipMemcpyDeviceToHost, c->stream));      // whole rows of the caller's matrix
    else HIPC(hipMemcpy2DAsync(dst, n_b * el, dev, nb * el, nb * el, na, hipMemcpyDeviceToHost, c->stream));
    return GEV_OK;
}
}
int gev_download_haps(gev_ctx* c, int pop, int chr, size_t row_begin, size_t n_rows, u64* bits, size_t row_stride_words)
{
    const char* who = "download_haps";
    GEVC(output_begin(c, pop, chr, who, true));
    PopState& P = c->pop[pop]; ChrStatic& S = P.cs[chr];
    GEVC(ensure_csr(c, pop));
    GEVC(check_range(who, "rows", row_begin, n_rows, 2 * P.n_people));
    GEVC(check_out(who, bits, n_rows, row_stride_words, ceil_div(S.L, 64), "words per row"));
    const size_t max_rows = output_chunk(c, 64u << 20, S.stride);
    GEVC(c->d_stage.ensure(std::min(max_rows, std::max<size_t>(n_rows, 1)) * S.stride, c->stream));
    for (size_t r0 = 0; r0 < n_rows; r0 += max_rows) {
        const size_t nr = std::min(max_rows, n_rows - r0);
        GEVC(stage_rows_mutated(c, P, chr, row_begin + r0, nr));
        GEVC(copy_out_rows(c, c->d_stage.p, S.stride, std::min(row_stride_words * 8, S.stride), nr, bits + r0 * row_stride_words, row_stride_words));
    }
    return GEV_OK;
}
// ---- K9: SNP-major outputs ---------------------------------------------------
int gev_download_snp_major(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, u64* bits, size_t row_stride_words)
{
    const char* who = "download_snp_major";
    GEVC(output_begin(c, pop, chr, who, true));
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, c->pop[pop].cs[chr].L));
    const size_t w = ceil_div(2 * c->pop[pop].n_people, 64);
    GEVC(check_out(who, bits, n_snps, row_stride_words, w, "words per row"));
    return snp_major_chunks(c, pop, chr, snp_begin, n_snps, w * 8, [&](size_t s, size_t ns, size_t stride) -> int {
        return copy_out_rows(c, c->d_snpmajor.p, stride * 8, w * 8, ns, bits + s * row_stride_words, row_stride_words);
    });
}
// bytes of the reference's .hap file for SNP lines [snp_begin, snp_begin+n_snps): n_snps * (4*n_people + 1)
int gev_format_hap_text(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, char* out, size_t out_bytes)
{
    GEVC(output_begin(c, pop, chr, "format_hap_text", true));
    const size_t rows = 2 * c->pop[pop].n_people, line = 2 * rows + 1;
    return format_snp_major(c, pop, chr, "format_hap_text", snp_begin, n_snps, line, line, out, out_bytes, [&](size_t ns, size_t stride) {
        hipLaunchKernelGGL(k_format_hap_text, dim3((unsigned)ceil_div(ceil_div(ns * line, 16), 256)), dim3(256), 0, c->stream, c->d_snpmajor.as<u64>(), stride, rows, (u32)ns, c->d_text.as<char>());
    });
}
// GT columns of the VCF data lines: n_snps * (4*n_people + 1) bytes; the caller writes the nine fixed columns in front
int gev_format_vcf_gt(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, char* out, size_t out_bytes)
{
    GEVC(output_begin(c, pop, chr, "format_vcf_gt", true));
    const size_t n_people = c->pop[pop].n_people, line = 4 * n_people + 1;
    return format_snp_major(c, pop, chr, "format_vcf_gt", snp_begin, n_snps, line, line, out, out_bytes, [&](size_t ns, size_t stride) {
        hipLaunchKernelGGL(k_format_vcf_gt, dim3((unsigned)ceil_div(ceil_div(ns * line, 16), 256)), dim3(256), 0, c->stream, c->d_snpmajor.as<u64>(), stride, n_people, (u32)ns, c->d_text.as<char>());
    });
}
// PLINK .bed body (SNP-major, without the 3 magic bytes 0x6c 0x1b 0x01): n_snps * ceil(n_people/4) bytes
int gev_format_bed(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, uint8_t* out, size_t out_bytes)
{
    GEVC(output_begin(c, pop, chr, "format_bed", true));
    const size_t n_people = c->pop[pop].n_people, bpl = ceil_div(n_people, 4);
    return format_snp_major(c, pop, chr, "format_bed", snp_begin, n_snps, bpl, ceil_div(2 * n_people, 64) * 8, out, out_bytes, [&](size_t ns, size_t stride) {
        hipLaunchKernelGGL(k_format_bed, dim3((unsigned)ceil_div(ns * bpl, 256)), dim3(256), 0, c->stream, c->d_snpmajor.as<u64>(), stride, n_people, (u32)ns, c->d_text.as<uint8_t>());
    });
}
// ---- genotype counts per SNP (gev_snpcount.h) -------------------------------------------------
// n_het / n_hom_alt of SNPs [snp_begin, +n_snps) over individuals [ind_begin, +n_ind): the plane pass reads the rows in place, the
// mutation overlay corrects the counts, both add into c->snp.cnt.  Nothing is staged, so gev_dbg_output_chunk has nothing to cap.
int gev_snp_genotype_counts(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind, uint32_t* n_het, uint32_t* n_hom_alt)
{
    const char* who = "snp_genotype_counts";
    GEVC(output_begin(c, pop, chr, who, true));
    PopState& P = c->pop[pop]; ChrStatic& S = P.cs[chr]; ChrState& cs = P.st[chr];
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, S.L));
    GEVC(check_range(who, "individuals", ind_begin, n_ind, P.n_people));
    if (n_snps && (!n_het || !n_hom_alt)) return fail(GEV_EINVAL, "%s: null output vector (n_het and n_hom_alt take %zu counts each)", who, n_snps);
    if (!n_snps) return GEV_OK;
    OptOut outs[2] = {{n_het, sizeof(u32), n_snps}, {n_hom_alt, sizeof(u32), n_snps}};
    if (!n_ind) { zero_outs(outs); return GEV_OK; }
    GEVC(ensure_csr(c, pop));                                           // the overlay reads whole lists
    hipStream_t st = c->stream;
    GEVC(c->snp.cnt.ensure(2 * n_snps, st));
    u32* d_het = c->snp.cnt; u32* d_hom = d_het + n_snps;
    outs[0].dev = d_het; outs[1].dev = d_hom;
    HIPC(hipMemsetAsync(d_het, 0, 2 * n_snps * sizeof(u32), st));
    const size_t q_first = snp_begin / SNPC_LOCI, n_q = (snp_begin + n_snps - 1) / SNPC_LOCI - q_first + 1;     // the chunks that hold a SNP of the range
    const size_t col_blocks = (q_first + n_q - 1) / SNPC_COLS - q_first / SNPC_COLS + 1;                        // the 64-chunk pieces of a row they lie in
    // blocks of individuals: several rounds of workgroups over the device (1024 are resident at a time) when the columns alone do
    // not give them, but every wave keeps a run of at least two counter periods, and a workgroup's packed partial stays in range
    const size_t min_ind = (size_t)SNPC_WAVES * 2 * (GEV_SNPC_F + 1);
    size_t splits = std::min(ceil_div(8192, col_blocks), std::max<size_t>(n_ind / min_ind, 1));
    size_t ind_per_block = ceil_div(n_ind, splits);
    if (ind_per_block > SNPC_MAX_IND) ind_per_block = SNPC_MAX_IND;
    splits = ceil_div(n_ind, ind_per_block);
    if (splits > 65535) return fail(GEV_EUNSUPPORTED, "%s: %zu individuals are more than one call counts", who, n_ind);
    const auto plane_pass = S.seg_shift >= 6 ? k_snp_counts<true> : k_snp_counts<false>;                        // a wave's 1 KiB of a row in one segment unit, or not
    hipLaunchKernelGGL(plane_pass, dim3((unsigned)col_blocks, (unsigned)splits), dim3(SNPC_WAVES * 64), 0, st, row_map(P, chr), ind_begin, n_ind, (u32)ind_per_block,
                       (u32)q_first, (u32)n_q, (u32)snp_begin, (u32)n_snps, d_het, d_hom);
    hipLaunchKernelGGL(k_snp_counts_apply_mut, dim3((unsigned)ceil_div(n_ind, 256)), dim3(256), 0, st, row_map(P, chr), ind_begin, n_ind,
                       cs.moff[P.cur], cs.mpos[P.cur], S.d_pos, (u32)snp_begin, (u32)n_snps, d_het, d_hom);
    KCHECK();
    return copy_back_outs(c, outs);
}
// the counter of gev_snpcount.h compiled for the host on haplotype-major rows in host memory: no device, no context
int gev_dbg_snp_counts_host(const uint64_t* bits, size_t row_stride_words, size_t n_ind, size_t L, size_t snp_begin, size_t n_snps,
                            uint32_t* n_het, uint32_t* n_hom_alt)
{
    const char* who = "dbg_snp_counts_host";
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, L));
    if (n_snps && (!n_het || !n_hom_alt)) return fail(GEV_EINVAL, "%s: null output vector", who);
    GEVC(check_host_rows(who, bits, row_stride_words, L, n_snps && n_ind));
    gev_snpc_count_rows_host(bits, row_stride_words, n_ind, snp_begin, n_snps, n_het, n_hom_alt);
    return GEV_OK;
}
// ---- the matrix-core products over bit planes (gev_bitprod.h): what the pair counts and LD share on the host --------
extern "C++" {      // (templates cannot have the C linkage of the block this file's functions sit in)
// One product of one sub-block of na x nb pairs with kernel k[large]: tiles of 128 x 128 pairs, or of 64 x 64 where fewer than `tiles`
// large ones have work and would leave compute units without a workgroup.  k[0]: the instantiation with FR = 2, k[1]: FR = 4.  The only
// place that knows the test mode of gev_dbg_bitprod_tiles and counts the launches
template <class K, class... Args>
static int bitprod_launch(gev_ctx* c, K* const (&k)[2], size_t na, size_t nb, size_t tiles, Args... args)
{
    if (!c->bp.n_cu) HIPC(hipDeviceGetAttribute(&c->bp.n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
    const bool large = c->bp.dbg_tiles ? c->bp.dbg_tiles == 2 : tiles >= (size_t)c->bp.n_cu;
    const unsigned tile = large ? BP_TILE : BP_TILE / 2;
    hipLaunchKernelGGL(k[large], dim3((unsigned)ceil_div(nb, tile), (unsigned)ceil_div(na, tile)), dim3(256), 0, c->stream, args...);
    KCHECK();
    c->bp.launches[large]++;
    return GEV_OK;
}
// the ten instantiations: [large]; [score][genotype][large]
static constexpr decltype(&k_pair_product<2>) pair_kernels[2] = {k_pair_product<2>, k_pair_product<4>};
static constexpr decltype(&k_ld_product<2, false, false>) ld_kernels[2][2][2] = {
    {{k_ld_product<2, false, false>, k_ld_product<4, false, false>}, {k_ld_product<2, true, false>, k_ld_product<4, true, false>}},
    {{k_ld_product<2, false, true>, k_ld_product<4, false, true>}, {k_ld_product<2, true, true>, k_ld_product<4, true, true>}}};
// A matrix of n_a x n_b pairs is walked in sub-blocks of at most blk rows a side (gev_dbg_output_chunk caps blk): side A of a block row
// is prepared once, side B once per sub-block -- O(rows) against the product's O(rows^2); the planes, not the staged rows, are what
// the product reads, so one staging buffer serves both sides.  prep(side_b, off, n, first) prepares rows [off, +n) of a side into its
// planes (first: these rows have not been prepared before in this call); products(na, nb, d_out) launches what fills the sub-block's
// results d_out[o] ([na][nb] in c->bp.out, null where outs[o] is).  They are copied into the caller's matrices outs[o] ([n_a][n_b],
// each may be null) and the stream is waited for, sub-block by sub-block.  With no matrix wanted only the sides are prepared: every
// block row of A and, where b_alone says that something of side B is wanted for itself, every block of B once
template <int NOUT, class Prep, class Products>
static int bitprod_walk(gev_ctx* c, size_t n_a, size_t n_b, size_t blk, const OptOut (&outs)[NOUT], bool b_alone, Prep prep, Products products)
{
    hipStream_t st = c->stream;
    bool want_mat = false;
    for (const OptOut& o : outs) want_mat = want_mat || o.host;
    GEVC(c->bp.out.ensure(NOUT * std::min(blk, n_a) * std::min(blk, n_b), st));
    for (size_t ia = 0; ia < n_a; ia += blk) {
        const size_t na = std::min(blk, n_a - ia);
        GEVC(prep(false, ia, na, true));
        for (size_t ib = 0; ib < n_b; ib += blk) {
            if (!want_mat && (ia || !b_alone)) break;                                         // only side B's vectors are left to make, once
            const size_t nb = std::min(blk, n_b - ib);
            GEVC(prep(true, ib, nb, ia == 0));
            if (want_mat) {
                u32* d_out[NOUT];
                for (int o = 0; o < NOUT; o++) d_out[o] = outs[o].host ? c->bp.out + (size_t)o * na * nb : nullptr;
                GEVC(products(na, nb, d_out));
                for (int o = 0; o < NOUT; o++) if (outs[o].host) GEVC(copy_out_block(c, outs[o].host, outs[o].el, n_b, ia, ib, na, nb, d_out[o]));
            }
            HIPC(hipStreamSynchronize(st));
        }
    }
    if (!want_mat) HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
}   // extern "C++"
// test hook: the tile size of the following products (0: by compute units, 1: 64 x 64, 2: 128 x 128, -1: as it is) and the launches so far
int gev_dbg_bitprod_tiles(gev_ctx* c, int mode, unsigned long long launches[2])
{
    GEVC(check_not_pending(c));
    if (mode < -1 || mode > 2) return fail(GEV_EINVAL, "dbg_bitprod_tiles: mode %d (0: by compute units, 1: tiles of 64 x 64, 2: tiles of 128 x 128, -1: unchanged)", mode);
    if (mode >= 0) c->bp.dbg_tiles = mode;
    if (launches) { launches[0] = c->bp.launches[0]; launches[1] = c->bp.launches[1]; }
    return GEV_OK;
}
// ---- genotype counts per individual and per pair of individuals (gev_paircount.h) ---------------
// individuals [ind0, +n) of a side staged through c->d_stage (ensure_csr has run) in passes of <= ~256 MB of rows and prepared:
// planes into `planes` (null: none; n_w4 words x n_pad individuals of x, then as many of y), counts into d_het / d_hom / d_wsum (each may be null; entry i = individual ind0 + i)
static int pair_prep_side(gev_ctx* c, PopState& P, int chr, size_t ind0, size_t n, size_t snp_begin, size_t n_snps, Dev<u64>* planes,
                          const u32* d_weight, u32* d_het, u32* d_hom, u64* d_wsum)
{
    ChrStatic& S = P.cs[chr];
    const size_t n_w4 = gev_bp_words4(snp_begin, n_snps), n_pad = planes ? round_up(n, BP_TILE) : n;
    const size_t pass = std::max<size_t>(output_chunk(c, 256u << 20, S.stride) / 2, 1);                       // (the units are rows, as in gev_download_haps)
    GEVC(c->d_stage.ensure(std::max<size_t>(2 * std::min(pass, n) * S.stride, 16), c->stream));
    u64 *px = nullptr, *py = nullptr;
    if (planes) { GEVC(planes->ensure(std::max<size_t>(2 * n_w4 * n_pad, 2), c->stream)); px = *planes; py = px + n_w4 * n_pad; }
    for (size_t off = 0; off < n; off += pass) {
        const size_t m = std::min(pass, n - off), cover = off + m == n ? n_pad - off : m;                     // the last pass zeroes the pad
        GEVC(stage_rows_mutated(c, P, chr, 2 * (ind0 + off), 2 * m));
        hipLaunchKernelGGL(k_pair_prep, dim3((unsigned)ceil_div(cover, 4)), dim3(256), 0, c->stream, c->d_stage.as<u64>(), S.stride / 8, (u32)m, (u32)cover,
                           (u32)off, (u32)n_pad, (u32)snp_begin, (u32)n_snps, (u32)n_w4, px, py, d_weight, d_het, d_hom, d_wsum);
        KCHECK();
    }
    return GEV_OK;
}
// what the two calls share: the opening, the three ranges, the width of a range
static int pair_begin(gev_ctx* c, int pop, int chr, const char* who, size_t snp_begin, size_t n_snps)
{
    GEVC(output_begin(c, pop, chr, who, true));
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, c->pop[pop].cs[chr].L));
    if (n_snps > GEV_PC_MAX_SNPS) return fail(GEV_EUNSUPPORTED, "%s: %zu SNPs in one call, at most %zu (a pair's dot product is a uint32)", who, n_snps, (size_t)GEV_PC_MAX_SNPS);
    return GEV_OK;
}
// individuals a side of a sub-block of the pair matrix: their words of the two planes within ~1 GB, at most 4096 (3 x 64 MB of results)
static size_t pair_block(const gev_ctx* c, size_t snp_begin, size_t n_snps)
{
    return std::min<size_t>(output_chunk(c, (size_t)1 << 30, 2 * gev_bp_words4(snp_begin, n_snps) * 8), 4096);
}
int gev_ind_genotype_counts(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind,
                            const uint32_t* weight, uint32_t* n_het, uint32_t* n_hom_alt, uint64_t* wsum)
{
    const char* who = "ind_genotype_counts";
    GEVC(pair_begin(c, pop, chr, who, snp_begin, n_snps));
    PopState& P = c->pop[pop];
    GEVC(check_range(who, "individuals", ind_begin, n_ind, P.n_people));
    if (!weight != !wsum) return fail(GEV_EINVAL, "%s: weights and wsum come together or not at all", who);
    if (!n_ind) return GEV_OK;
    OptOut outs[3] = {{n_het, sizeof(u32), n_ind}, {n_hom_alt, sizeof(u32), n_ind}, {wsum, sizeof(u64), n_ind}};
    if (!n_snps) { zero_outs(outs); return GEV_OK; }
    GEVC(ensure_csr(c, pop));
    hipStream_t st = c->stream;
    const u32* d_weight = nullptr;
    if (weight) {
        GEVC(c->bp.pair_w.ensure(n_snps, st));
        HIPC(hipMemcpyAsync(c->bp.pair_w.p, weight, n_snps * sizeof(u32), hipMemcpyHostToDevice, st));
        d_weight = c->bp.pair_w;
    }
    GEVC(c->bp.cnt.ensure(n_ind * 16, st));
    u64* d_ws = c->bp.cnt.as<u64>(); u32* d_het = (u32*)(d_ws + n_ind); u32* d_hom = d_het + n_ind;
    outs[0].dev = d_het; outs[1].dev = d_hom; outs[2].dev = d_ws;
    GEVC(pair_prep_side(c, P, chr, ind_begin, n_ind, snp_begin, n_snps, nullptr, d_weight, d_het, d_hom, wsum ? d_ws : nullptr));
    return copy_back_outs(c, outs);
}
// The pair matrix is walked in sub-blocks of at most pair_block() individuals a side (bitprod_walk; gev_dbg_output_chunk caps them, and the
// rows of a staging pass), each side staged and prepared through c->d_stage.
int gev_pair_genotype_counts(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, size_t a_begin, size_t n_a, size_t b_begin, size_t n_b,
                             uint32_t* n_hethet, uint32_t* n_opphom, uint32_t* dot)
{
    const char* who = "pair_genotype_counts";
    GEVC(pair_begin(c, pop, chr, who, snp_begin, n_snps));
    PopState& P = c->pop[pop];
    GEVC(check_range(who, "individuals (a)", a_begin, n_a, P.n_people));
    GEVC(check_range(who, "individuals (b)", b_begin, n_b, P.n_people));
    if (!n_a || !n_b) return GEV_OK;
    const OptOut outs[3] = {{n_hethet, sizeof(u32), n_a * n_b}, {n_opphom, sizeof(u32), n_a * n_b}, {dot, sizeof(u32), n_a * n_b}};
    if (!n_snps) { zero_outs(outs); return GEV_OK; }
    if (!n_hethet && !n_opphom && !dot) return GEV_OK;
    GEVC(ensure_csr(c, pop));
    hipStream_t st = c->stream;
    const size_t blk = pair_block(c, snp_begin, n_snps), ba = std::min(blk, n_a), n_w4 = gev_bp_words4(snp_begin, n_snps);
    GEVC(c->bp.cnt.ensure((ba + std::min(blk, n_b)) * sizeof(u32), st));
    u32* d_hom_a = c->bp.cnt.as<u32>(); u32* d_hom_b = d_hom_a + ba;
    return bitprod_walk(c, n_a, n_b, blk, outs, false,
        [&](bool side_b, size_t off, size_t n, bool) -> int {
            return pair_prep_side(c, P, chr, (side_b ? b_begin : a_begin) + off, n, snp_begin, n_snps, side_b ? &c->bp.b : &c->bp.a, nullptr, nullptr, side_b ? d_hom_b : d_hom_a, nullptr);
        },
        [&](size_t na, size_t nb, u32* const* d_out) -> int {
            const size_t pad_a = round_up(na, BP_TILE), pad_b = round_up(nb, BP_TILE);
            const u64 *xa = c->bp.a, *xb = c->bp.b;
            return bitprod_launch(c, pair_kernels, na, nb, (pad_a / BP_TILE) * (pad_b / BP_TILE), xa, xa + n_w4 * pad_a, (u32)pad_a, xb, xb + n_w4 * pad_b, (u32)pad_b, (u32)n_w4,
                                  (const u32*)d_hom_a, (const u32*)d_hom_b, (u32)na, (u32)nb, d_out[0], d_out[1], d_out[2]);
        });
}
// the arithmetic of gev_paircount.h compiled for the host on haplotype-major rows in host memory: no device, no context
int gev_dbg_pair_counts_host(const uint64_t* bits, size_t row_stride_words, size_t n_ind, size_t L, size_t snp_begin, size_t n_snps,
                             size_t a_begin, size_t n_a, size_t b_begin, size_t n_b,
                             uint32_t* n_het, uint32_t* n_hom_alt, uint32_t* n_hethet, uint32_t* n_opphom, uint32_t* dot)
{
    const char* who = "dbg_pair_counts_host";
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, L));
    if (n_snps > GEV_PC_MAX_SNPS) return fail(GEV_EUNSUPPORTED, "%s: %zu SNPs in one call, at most %zu (a pair's dot product is a uint32)", who, n_snps, (size_t)GEV_PC_MAX_SNPS);
    GEVC(check_range(who, "individuals (a)", a_begin, n_a, n_ind));
    GEVC(check_range(who, "individuals (b)", b_begin, n_b, n_ind));
    GEVC(check_host_rows(who, bits, row_stride_words, L, n_snps && n_ind));
    const bool pairs = n_a && n_b;
    gev_pc_counts_host(bits, row_stride_words, n_ind, snp_begin, n_snps, a_begin, pairs ? n_a : 0, b_begin, pairs ? n_b : 0, n_het, n_hom_alt,
                       pairs ? n_hethet : nullptr, pairs ? n_opphom : nullptr, pairs ? dot : nullptr);
    return GEV_OK;
}
// ---- linkage disequilibrium per pair of SNPs (gev_ldcount.h) ------------------------------------
// SNPs a side of a sub-block of the SNP-pair matrix: their words of the plane within ~1 GB, their SNP-major rows within the ~256 MB of
// one snp_major_device pass (so a side is one pass), at most 4096 (2 x 64 MB of results)
static size_t ld_block(const gev_ctx* c, size_t n_people, size_t ind_begin, size_t n_ind)
{
    const size_t plane = output_chunk(c, (size_t)1 << 30, gev_bp_words4(2 * ind_begin, 2 * n_ind) * 8);
    return std::min(std::min(plane, output_chunk(c, 256u << 20, ceil_div(2 * n_people, 64) * 8)), (size_t)4096);
}
struct LdSide { const u64* plane; u32 *c, *het, *hom; size_t n_pad; };
// SNPs [s0, +n) of (pop, chr) through c->d_snpmajor into `planes` over individuals [ind_begin, +n_ind), their counts into the three
// vectors of cnt_stride entries at d_cnt
static int ld_prep_side(gev_ctx* c, int pop, int chr, size_t s0, size_t n, size_t ind_begin, size_t n_ind, Dev<u64>& planes, u32* d_cnt, size_t cnt_stride, LdSide& side)
{
    const size_t n_w4 = gev_bp_words4(2 * ind_begin, 2 * n_ind), n_pad = round_up(n, BP_TILE);
    size_t stride;
    GEVC(planes.ensure(std::max<size_t>(n_w4 * n_pad, 2), c->stream));
    GEVC(snp_major_device(c, pop, chr, s0, n, stride));
    side = LdSide{planes, d_cnt, d_cnt + cnt_stride, d_cnt + 2 * cnt_stride, n_pad};
    hipLaunchKernelGGL(k_ld_prep, dim3((unsigned)ceil_div(n_pad, 4)), dim3(256), 0, c->stream, c->d_snpmajor.as<u64>(), stride, (u32)n, (u32)n_pad, 0u, (u32)n_pad,
                       (u64)(2 * ind_begin), (u64)(2 * n_ind), (u32)n_w4, planes, side.c, side.het, side.hom);
    KCHECK();
    return GEV_OK;
}
// The SNP-pair matrix is walked in sub-blocks of at most ld_block() SNPs a side (bitprod_walk; gev_dbg_output_chunk caps them, and with them
// the SNPs of a snp_major_device pass), each side prepared through c->d_snpmajor, which so serves both sides and both chromosomes.
int gev_ld_counts(gev_ctx* c, int pop, int chr_a, size_t a_begin, size_t n_a, int chr_b, size_t b_begin, size_t n_b, size_t ind_begin, size_t n_ind,
                  uint32_t* n11, uint32_t* gg, uint32_t* c_a, uint32_t* het_a, uint32_t* hom_a, uint32_t* c_b, uint32_t* het_b, uint32_t* hom_b)
{
    const char* who = "ld_counts";
    GEVC(output_begin(c, pop, chr_a, who, true));
    if (chr_b != chr_a) GEVC(output_begin(c, pop, chr_b, who, true));
    PopState& P = c->pop[pop];
    GEVC(check_range(who, "SNPs (a)", a_begin, n_a, P.cs[chr_a].L));
    GEVC(check_range(who, "SNPs (b)", b_begin, n_b, P.cs[chr_b].L));
    GEVC(check_range(who, "individuals", ind_begin, n_ind, P.n_people));
    if (n_ind > GEV_LD_MAX_IND) return fail(GEV_EUNSUPPORTED, "%s: %zu individuals in one call, at most %zu (a pair's genotype product is a uint32)", who, n_ind, (size_t)GEV_LD_MAX_IND);
    if (!n_a || !n_b) return GEV_OK;
    uint32_t* const vec_a[3] = {c_a, het_a, hom_a}; uint32_t* const vec_b[3] = {c_b, het_b, hom_b};
    const OptOut mats[2] = {{n11, sizeof(u32), n_a * n_b}, {gg, sizeof(u32), n_a * n_b}};
    if (!n_ind) {
        zero_outs(mats);
        for (uint32_t* o : vec_a) if (o) memset(o, 0, n_a * sizeof(u32));
        for (uint32_t* o : vec_b) if (o) memset(o, 0, n_b * sizeof(u32));
        return GEV_OK;
    }
    const bool want_mat = n11 || gg, want_b = c_b || het_b || hom_b;
    if (!want_mat && !want_b && !c_a && !het_a && !hom_a) return GEV_OK;
    hipStream_t st = c->stream;
    const size_t blk = ld_block(c, P.n_people, ind_begin, n_ind), ba = std::min(blk, n_a), bb = std::min(blk, n_b);
    const size_t n_w4 = gev_bp_words4(2 * ind_begin, 2 * n_ind);
    GEVC(c->bp.cnt.ensure(3 * (ba + bb) * sizeof(u32), st));
    u32* d_cnt_a = c->bp.cnt.as<u32>(); u32* d_cnt_b = d_cnt_a + 3 * ba;
    LdSide A, B;
    return bitprod_walk(c, n_a, n_b, blk, mats, want_b,
        [&](bool side_b, size_t off, size_t n, bool first) -> int {                           // a side's vectors come back the first time its SNPs are prepared
            LdSide& S = side_b ? B : A; uint32_t* const* vec = side_b ? vec_b : vec_a;
            if (side_b) GEVC(ld_prep_side(c, pop, chr_b, b_begin + off, n, ind_begin, n_ind, c->bp.b, d_cnt_b, bb, S));
            else GEVC(ld_prep_side(c, pop, chr_a, a_begin + off, n, ind_begin, n_ind, c->bp.a, d_cnt_a, ba, S));
            u32* const d_vec[3] = {S.c, S.het, S.hom};
            for (int o = 0; o < 3 && first; o++) if (vec[o]) HIPC(hipMemcpyAsync(vec[o] + off, d_vec[o], n * sizeof(u32), hipMemcpyDeviceToHost, st));
            return GEV_OK;
        },
        [&](size_t na, size_t nb, u32* const* d_out) -> int {
            for (int o = 0; o < 2; o++) if (mats[o].host) GEVC(bitprod_launch(c, ld_kernels[0][o], na, nb, (A.n_pad / BP_TILE) * (B.n_pad / BP_TILE), A.plane, (u32)A.n_pad, B.plane, (u32)B.n_pad, (u32)n_w4, (u32)na, (u32)nb, d_out[o], LdScoreArgs{}));
            return GEV_OK;
        });
}
// the windows of SNPs [snp_begin, +n_snps) of a chromosome of L SNPs: both arrays non-decreasing, win_lo[t] <= snp_begin + t < win_hi[t] <= L
static int ld_check_windows(const char* who, size_t snp_begin, size_t n_snps, const uint32_t* win_lo, const uint32_t* win_hi, size_t L)
{
    if (n_snps && (!win_lo || !win_hi)) return fail(GEV_EINVAL, "%s: null window array (win_lo and win_hi take %zu entries each)", who, n_snps);
    for (size_t t = 0; t < n_snps; t++) {
        const size_t j = snp_begin + t;
        if (win_lo[t] > j || win_hi[t] <= j || win_hi[t] > L) return fail(GEV_EINVAL, "%s: window [%u,%u) of SNP %zu does not hold it or ends beyond the %zu SNPs there are", who, win_lo[t], win_hi[t], j, L);
        if (t && (win_lo[t] < win_lo[t - 1] || win_hi[t] < win_hi[t - 1])) return fail(GEV_EINVAL, "%s: window [%u,%u) of SNP %zu begins or ends before the one in front of it", who, win_lo[t], win_hi[t], j);
    }
    return GEV_OK;
}
// The band is walked in the same sub-blocks: for a block row of SNPs, side B runs over the union of their windows (the windows are
// non-decreasing: from the first one's begin to the last one's end) and no further; within a sub-block a wave whose pairs lie outside
// the band leaves at once.  The quanta are added on the device; what comes back are the two vectors.
int gev_ld_scores(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, const uint32_t* win_lo, const uint32_t* win_hi,
                  size_t ind_begin, size_t n_ind, int genotype, uint64_t* score_q40, uint32_t* n_terms)
{
    const char* who = "ld_scores";
    GEVC(output_begin(c, pop, chr, who, true));
    PopState& P = c->pop[pop];
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, P.cs[chr].L));
    GEVC(check_range(who, "individuals", ind_begin, n_ind, P.n_people));
    if (n_ind > GEV_LD_MAX_IND) return fail(GEV_EUNSUPPORTED, "%s: %zu individuals in one call, at most %zu (a pair's genotype product is a uint32)", who, n_ind, (size_t)GEV_LD_MAX_IND);
    GEVC(ld_check_windows(who, snp_begin, n_snps, win_lo, win_hi, P.cs[chr].L));
    if (!n_snps || (!score_q40 && !n_terms)) return GEV_OK;
    OptOut outs[2] = {{score_q40, sizeof(u64), n_snps}, {n_terms, sizeof(u32), n_snps}};
    if (!n_ind) { zero_outs(outs); return GEV_OK; }
    hipStream_t st = c->stream;
    const size_t blk = ld_block(c, P.n_people, ind_begin, n_ind), ba = std::min(blk, n_snps), bb = std::min<size_t>(blk, P.cs[chr].L);
    const size_t n_w4 = gev_bp_words4(2 * ind_begin, 2 * n_ind);
    GEVC(c->bp.cnt.ensure(3 * (ba + bb) * sizeof(u32), st));
    GEVC(c->bp.ld_win.ensure(2 * n_snps, st));
    GEVC(c->bp.ld_score.ensure(n_snps * (sizeof(u64) + sizeof(u32)), st));
    u32* d_cnt_a = c->bp.cnt.as<u32>(); u32* d_cnt_b = d_cnt_a + 3 * ba;
    u32* d_lo = c->bp.ld_win; u32* d_hi = d_lo + n_snps;
    u64* d_score = c->bp.ld_score.as<u64>(); u32* d_terms = (u32*)(d_score + n_snps);
    outs[0].dev = d_score; outs[1].dev = d_terms;
    HIPC(hipMemcpyAsync(d_lo, win_lo, n_snps * sizeof(u32), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_hi, win_hi, n_snps * sizeof(u32), hipMemcpyHostToDevice, st));
    HIPC(hipMemsetAsync(d_score, 0, n_snps * (sizeof(u64) + sizeof(u32)), st));
    for (size_t ia = 0; ia < n_snps; ia += blk) {
        const size_t na = std::min(blk, n_snps - ia);
        LdSide A, B;
        GEVC(ld_prep_side(c, pop, chr, snp_begin + ia, na, ind_begin, n_ind, c->bp.a, d_cnt_a, ba, A));
        const size_t u0 = win_lo[ia], u1 = win_hi[ia + na - 1];
        for (size_t ib = u0; ib < u1; ib += blk) {
            const size_t nb = std::min(blk, u1 - ib);
            GEVC(ld_prep_side(c, pop, chr, ib, nb, ind_begin, n_ind, c->bp.b, d_cnt_b, bb, B));
            const LdScoreArgs sa{A.c, A.het, A.hom, B.c, B.het, B.hom, d_lo + ia, d_hi + ia, d_score + ia, d_terms + ia, (u64)n_ind, (u32)ib};
            size_t band_tiles = 0;                                                             // the large tiles of the sub-block that the band touches
            for (size_t r0 = 0; r0 < na; r0 += BP_TILE) {
                const size_t k0 = std::max<size_t>(win_lo[ia + r0], ib), k1 = std::min<size_t>(win_hi[ia + std::min<size_t>(r0 + BP_TILE, na) - 1], ib + nb);
                if (k1 > k0) band_tiles += (k1 - 1 - ib) / BP_TILE - (k0 - ib) / BP_TILE + 1;
            }
            if (!band_tiles) continue;
            GEVC(bitprod_launch(c, ld_kernels[1][genotype != 0], na, nb, band_tiles / LD_SCORE_TILES_PER_CU, A.plane, (u32)A.n_pad, B.plane, (u32)B.n_pad, (u32)n_w4, (u32)na, (u32)nb, (u32*)nullptr, sa));
        }
    }
    return copy_back_outs(c, outs);
}
// the arithmetic of gev_ldcount.h compiled for the host on haplotype-major rows in host memory: no device, no context.  The block form
// (SNPs [a_begin, +n_a) of rows_a against [b_begin, +n_b) of rows_b) and, with windows, the score form over side A's rows
int gev_dbg_ld_host(const uint64_t* bits_a, size_t stride_a, size_t L_a, const uint64_t* bits_b, size_t stride_b, size_t L_b, size_t n_people,
                    size_t a_begin, size_t n_a, size_t b_begin, size_t n_b, size_t ind_begin, size_t n_ind,
                    uint32_t* n11, uint32_t* gg, uint32_t* c_a, uint32_t* het_a, uint32_t* hom_a, uint32_t* c_b, uint32_t* het_b, uint32_t* hom_b,
                    const uint32_t* win_lo, const uint32_t* win_hi, int genotype, uint64_t* score_q40, uint32_t* n_terms)
{
    const char* who = "dbg_ld_host";
    GEVC(check_range(who, "SNPs (a)", a_begin, n_a, L_a));
    GEVC(check_range(who, "SNPs (b)", b_begin, n_b, L_b));
    GEVC(check_range(who, "individuals", ind_begin, n_ind, n_people));
    if (n_ind > GEV_LD_MAX_IND) return fail(GEV_EUNSUPPORTED, "%s: %zu individuals in one call, at most %zu (a pair's genotype product is a uint32)", who, n_ind, (size_t)GEV_LD_MAX_IND);
    const bool scores = win_lo || win_hi || score_q40 || n_terms;
    if (scores) GEVC(ld_check_windows(who, a_begin, n_a, win_lo, win_hi, L_a));
    if (n_ind && n_a && (!bits_a || stride_a < ceil_div(L_a, 64))) return fail(GEV_EINVAL, "%s: rows (a) of %zu words, %zu needed", who, stride_a, ceil_div(L_a, 64));
    if (n_ind && n_a && n_b && (!bits_b || stride_b < ceil_div(L_b, 64))) return fail(GEV_EINVAL, "%s: rows (b) of %zu words, %zu needed", who, stride_b, ceil_div(L_b, 64));
    if (n_a && n_b) gev_ld_counts_host(bits_a, stride_a, a_begin, n_a, bits_b, stride_b, b_begin, n_b, ind_begin, n_ind, n11, gg, c_a, het_a, hom_a, c_b, het_b, hom_b);
    if (scores) gev_ld_scores_host(bits_a, stride_a, a_begin, n_a, win_lo, win_hi, ind_begin, n_ind, genotype != 0, score_q40, n_terms);
    return GEV_OK;
}
// gev_ld_r2_q40 alone, compiled for the host, on n triples
int gev_dbg_ld_r2_q40_host(const int64_t* num, const uint64_t* den_j, const uint64_t* den_k, size_t n, uint64_t* q40)
{
    if (n && (!num || !den_j || !den_k || !q40)) return fail(GEV_EINVAL, "dbg_ld_r2_q40_host: null array");
    for (size_t i = 0; i < n; i++) q40[i] = gev_ld_r2_q40(num[i], den_j[i], den_k[i]);
    return GEV_OK;
}
// ---- the signed digit-column product under trait sums and scores (gev_digitprod.h) ---------------
struct DpNouns { const char *array, *column, *columns, *value, *values, *entry, *entries; };   // what a feature's refusals call its columns
static const DpNouns TS_NOUNS = {"trait", "trait", "traits", "quantum", "quanta", "individual", "individuals"};
static const DpNouns IS_NOUNS = {"weight", "column", "columns", "weight", "weights", "SNP", "SNPs"};
// val: [n_cols][n], n the summed entries of a row
static int dp_check_columns(const char* who, const DpNouns& nn, const int32_t* val, size_t n_cols, size_t n)
{
    if (n > GEV_DP_MAX_N) return fail(GEV_EUNSUPPORTED, "%s: %zu %s in one call, at most %zu (a digit's sum is an int32)", who, n, nn.entries, (size_t)GEV_DP_MAX_N);
    if (!n_cols || !n) return GEV_OK;
    if (!val) return fail(GEV_EINVAL, "%s: null %s array (%zu %s of %zu %s each)", who, nn.array, n_cols, nn.columns, n, nn.values);
    for (size_t i = 0; i < n_cols * n; i++)
        if (val[i] > GEV_DP_MAX_VAL || val[i] < -GEV_DP_MAX_VAL) return fail(GEV_EINVAL, "%s: %s %d of %s %zu, %s %zu beyond +-2^30", who, nn.value, val[i], nn.column, i / n, nn.entry, i % n);
    return GEV_OK;
}
// Side B of a call: the columns uploaded and turned by the feature's preparation kernel (k_ts_prep, k_is_prep: a thread per 16-byte fragment,
// `frags` of them per word of the n_w4 summed) into the operand bytes that serve every block; the partials and sums of a block of at most blk rows
static int dp_operand(gev_ctx* c, void (*k_prep)(const int32_t*, u32, u64, u64, u32, u32, uint4*), const int32_t* val, size_t n_cols, size_t begin, size_t n,
                      size_t n_w4, size_t frags, size_t blk)
{
    hipStream_t st = c->stream;
    const size_t n_cg = ceil_div(n_cols, 4);
    GEVC(c->dp.val.ensure(n_cols * n, st));
    GEVC(c->dp.b.ensure(n_cg * n_w4 * frags, st));
    GEVC(c->dp.acc.ensure(2 * n_cg * round_up(blk, BP_TILE) * 16, st));
    GEVC(c->dp.out.ensure(2 * n_cols * blk, st));
    HIPC(hipMemcpyAsync(c->dp.val.p, val, n_cols * n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_prep, dim3((unsigned)ceil_div(n_cg * n_w4 * frags, 256)), dim3(256), 0, st, c->dp.val, (u32)n_cols, (u64)begin, (u64)n, (u32)n_w4, (u32)n_cg, c->dp.b);
    KCHECK();
    return GEV_OK;
}
// The n_rows rows of the product in blocks of blk: prep(off, n) prepares side A of rows [off, +n), padded to BP_TILE rows as ld_prep_side and
// pair_prep_side pad them; product(n_pad, cg0, n_z) launches the feature's product kernel for column groups [cg0, +n_z) (a grid's z).  Where a
// matrix of mats ([n_cols][n_rows] int64 on the host) is wanted a block's sums are finished and copied out before the next block's kernels run
// (stream order); the call returns when the last ones have arrived
extern "C++" template <class Prep, class Product>
static int dp_walk(gev_ctx* c, size_t n_rows, size_t blk, size_t n_cols, const OptOut* mats, Prep prep, Product product)
{
    hipStream_t st = c->stream;
    const size_t n_cg = ceil_div(n_cols, 4);
    for (size_t off = 0; off < n_rows; off += blk) {
        const size_t n = std::min(blk, n_rows - off), n_pad = round_up(n, BP_TILE);
        GEVC(prep(off, n));
        if (!n_cols || (!mats[0].host && !mats[1].host)) continue;
        HIPC(hipMemsetAsync(c->dp.acc.p, 0, 2 * n_cg * n_pad * 16 * sizeof(int), st));
        for (size_t cg0 = 0; cg0 < n_cg; cg0 += 65535) product(n_pad, cg0, std::min<size_t>(n_cg - cg0, 65535));
        hipLaunchKernelGGL(k_dp_finish, dim3((unsigned)ceil_div(2 * n_cols * n, 256)), dim3(256), 0, st, c->dp.acc, (u32)n_pad, (u32)n_cg,
                           (u32)n_cols, (u32)n, (u32)blk, c->dp.out);
        KCHECK();
        for (int o = 0; o < 2; o++)
            if (mats[o].host) HIPC(hipMemcpy2DAsync((int64_t*)mats[o].host + off, n_rows * sizeof(int64_t), c->dp.out + (size_t)o * n_cols * blk, blk * sizeof(int64_t),
                                                    n * sizeof(int64_t), n_cols, hipMemcpyDeviceToHost, st));
    }
    HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
// ---- trait sums per SNP (gev_traitsum.h) -------------------------------------------------------
// The SNPs are walked in blocks of at most ld_block() (gev_dbg_output_chunk caps them): a block is one snp_major_device pass and one
// k_ld_prep into c->bp.a, its counts copied out behind it; the traits' operand bytes are made once per call
int gev_snp_trait_sums(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind,
                       const int32_t* trait, size_t n_traits, int64_t* gsum, int64_t* hetsum, uint32_t* n_het, uint32_t* n_hom_alt)
{
    const char* who = "snp_trait_sums";
    GEVC(output_begin(c, pop, chr, who, true));
    PopState& P = c->pop[pop];
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, P.cs[chr].L));
    GEVC(check_range(who, "individuals", ind_begin, n_ind, P.n_people));
    GEVC(dp_check_columns(who, TS_NOUNS, trait, n_traits, n_ind));
    if (!n_snps) return GEV_OK;
    const OptOut outs[4] = {{gsum, sizeof(int64_t), n_traits * n_snps}, {hetsum, sizeof(int64_t), n_traits * n_snps}, {n_het, sizeof(u32), n_snps}, {n_hom_alt, sizeof(u32), n_snps}};
    if (!n_ind) { zero_outs(outs); return GEV_OK; }
    const bool want_sums = (gsum || hetsum) && n_traits;
    if (!want_sums && !n_het && !n_hom_alt) return GEV_OK;
    hipStream_t st = c->stream;
    const size_t blk = std::min(ld_block(c, P.n_people, ind_begin, n_ind), n_snps);
    const size_t n_w4 = gev_bp_words4(2 * ind_begin, 2 * n_ind), n_cg = ceil_div(n_traits, 4), slices = ceil_div(n_w4, GEV_TS_SLICE_W);
    GEVC(c->bp.cnt.ensure(3 * blk * sizeof(u32), st));
    if (want_sums) GEVC(dp_operand(c, k_ts_prep, trait, n_traits, ind_begin, n_ind, n_w4, 32, blk));   // 32 individuals x 16 columns a word: 512 bytes
    LdSide A;
    return dp_walk(c, n_snps, blk, n_traits, outs,
        [&](size_t off, size_t n) -> int {
            GEVC(ld_prep_side(c, pop, chr, snp_begin + off, n, ind_begin, n_ind, c->bp.a, c->bp.cnt.as<u32>(), blk, A));
            if (n_het) HIPC(hipMemcpyAsync(n_het + off, A.het, n * sizeof(u32), hipMemcpyDeviceToHost, st));
            if (n_hom_alt) HIPC(hipMemcpyAsync(n_hom_alt + off, A.hom, n * sizeof(u32), hipMemcpyDeviceToHost, st));
            return GEV_OK;
        },
        [&](size_t n_pad, size_t cg0, size_t n_z) {
            hipLaunchKernelGGL(k_ts_product, dim3((unsigned)(n_pad / BP_TILE), (unsigned)slices, (unsigned)n_z), dim3(256), 0, st,
                               A.plane, (u32)n_pad, (u32)n_w4, c->dp.b, (u32)n_cg, (u32)cg0, c->dp.acc);
        });
}
// the arithmetic of gev_traitsum.h compiled for the host on haplotype-major rows in host memory: no device, no context
int gev_dbg_trait_sums_host(const uint64_t* bits, size_t row_stride_words, size_t n_people, size_t L, size_t snp_begin, size_t n_snps,
                            size_t ind_begin, size_t n_ind, const int32_t* trait, size_t n_traits,
                            int64_t* gsum, int64_t* hetsum, uint32_t* n_het, uint32_t* n_hom_alt)
{
    const char* who = "dbg_trait_sums_host";
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, L));
    GEVC(check_range(who, "individuals", ind_begin, n_ind, n_people));
    GEVC(dp_check_columns(who, TS_NOUNS, trait, n_traits, n_ind));
    GEVC(check_host_rows(who, bits, row_stride_words, L, n_snps && n_ind));
    if (!n_snps) return GEV_OK;
    const OptOut outs[4] = {{gsum, sizeof(int64_t), n_traits * n_snps}, {hetsum, sizeof(int64_t), n_traits * n_snps}, {n_het, sizeof(u32), n_snps}, {n_hom_alt, sizeof(u32), n_snps}};
    if (!n_ind) { zero_outs(outs); return GEV_OK; }
    gev_trait_sums_host(bits, row_stride_words, snp_begin, n_snps, ind_begin, n_ind, trait, n_traits, gsum, hetsum, n_het, n_hom_alt);
    return GEV_OK;
}
// ---- scores per individual (gev_indscore.h) ----------------------------------------------------
// The individuals are walked in blocks (gev_dbg_output_chunk caps them, and the rows of a staging pass): their words of the two planes within
// ~1 GB as pair_block() has it, at most 65536 (2 KB of partials each at 64 columns); a block is one pair_prep_side into c->bp.a; the weights'
// operand bytes are made once per call
int gev_ind_scores(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind,
                   const int32_t* weight, size_t n_scores, int64_t* gscore, int64_t* hetscore)
{
    const char* who = "ind_scores";
    GEVC(output_begin(c, pop, chr, who, true));
    PopState& P = c->pop[pop];
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, P.cs[chr].L));
    GEVC(check_range(who, "individuals", ind_begin, n_ind, P.n_people));
    GEVC(dp_check_columns(who, IS_NOUNS, weight, n_scores, n_snps));
    if (!n_ind) return GEV_OK;
    const OptOut outs[2] = {{gscore, sizeof(int64_t), n_scores * n_ind}, {hetscore, sizeof(int64_t), n_scores * n_ind}};
    if (!n_snps || !n_scores) { zero_outs(outs); return GEV_OK; }
    if (!gscore && !hetscore) return GEV_OK;
    GEVC(ensure_csr(c, pop));
    hipStream_t st = c->stream;
    const size_t n_w4 = gev_bp_words4(snp_begin, n_snps), blk = std::min(std::min<size_t>(output_chunk(c, (size_t)1 << 30, 2 * n_w4 * 8), 65536), n_ind), n_cg = ceil_div(n_scores, 4), slices = ceil_div(n_w4, GEV_IS_SLICE_W);
    GEVC(dp_operand(c, k_is_prep, weight, n_scores, snp_begin, n_snps, n_w4, 64, blk));                // 64 SNPs x 16 columns a word: 1 KiB
    return dp_walk(c, n_ind, blk, n_scores, outs,
        [&](size_t off, size_t n) { return pair_prep_side(c, P, chr, ind_begin + off, n, snp_begin, n_snps, &c->bp.a, nullptr, nullptr, nullptr, nullptr); },
        [&](size_t n_pad, size_t cg0, size_t n_z) {
            const u64* px = c->bp.a;
            hipLaunchKernelGGL(k_is_product, dim3((unsigned)(n_pad / BP_TILE), (unsigned)slices, (unsigned)n_z), dim3(256), 0, st,
                               px, px + n_w4 * n_pad, (u32)n_pad, (u32)n_w4, c->dp.b, (u32)n_cg, (u32)cg0, c->dp.acc);
        });
}
// the arithmetic of gev_indscore.h compiled for the host on haplotype-major rows in host memory: no device, no context
int gev_dbg_ind_scores_host(const uint64_t* bits, size_t row_stride_words, size_t n_people, size_t L, size_t snp_begin, size_t n_snps,
                            size_t ind_begin, size_t n_ind, const int32_t* weight, size_t n_scores, int64_t* gscore, int64_t* hetscore)
{
    const char* who = "dbg_ind_scores_host";
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, L));
    GEVC(check_range(who, "individuals", ind_begin, n_ind, n_people));
    GEVC(dp_check_columns(who, IS_NOUNS, weight, n_scores, n_snps));
    GEVC(check_host_rows(who, bits, row_stride_words, L, n_snps && n_ind));
    if (!n_ind) return GEV_OK;
    const OptOut outs[2] = {{gscore, sizeof(int64_t), n_scores * n_ind}, {hetscore, sizeof(int64_t), n_scores * n_ind}};
    if (!n_snps || !n_scores) { zero_outs(outs); return GEV_OK; }
    gev_ind_scores_host(bits, row_stride_words, snp_begin, n_snps, ind_begin, n_ind, weight, n_scores, gscore, hetscore);
    return GEV_OK;
}
// ---- identity by descent per pair of haplotype rows, base pairs by root population (gev_ibd.h) ----------------
// what the two calls begin with, for one population: the opening of gev_format_interval_text
static int ibd_begin(gev_ctx* c, int pop, int chr, const char* who)
{
    GEVC(output_begin(c, pop, chr, who, false));
    if (!c->track_intervals) return fail(GEV_ESTATE, "%s: interval tracking is disabled (gev_set_track_intervals)", who);
    return ensure_csr(c, pop);
}
// The pair matrix is walked in sub-blocks of at most 4096 rows a side (gev_dbg_output_chunk caps them): a sub-block is one launch of
// k_ibd_tiles into c->ibd.out, copied into the caller's matrices before the next one's kernel runs.
int gev_ibd_sharing(gev_ctx* c, int chr, int pop_a, size_t a_begin, size_t n_a, int pop_b, size_t b_begin, size_t n_b,
                    uint64_t min_bp, uint64_t* shared_bp, uint32_t* n_seg, uint64_t* max_seg)
{
    const char* who = "ibd_sharing";
    GEVC(ibd_begin(c, pop_a, chr, who));
    if (pop_b != pop_a) GEVC(ibd_begin(c, pop_b, chr, who));
    PopState &PA = c->pop[pop_a], &PB = c->pop[pop_b];
    GEVC(check_range(who, "rows (a)", a_begin, n_a, 2 * PA.n_people));
    GEVC(check_range(who, "rows (b)", b_begin, n_b, 2 * PB.n_people));
    if (!n_a || !n_b || (!shared_bp && !n_seg && !max_seg)) return GEV_OK;
    hipStream_t st = c->stream;
    const u32* poff_a = PA.st[chr].poff[PA.cur]; const gev_part* parts_a = PA.st[chr].parts[PA.cur];
    const u32* poff_b = PB.st[chr].poff[PB.cur]; const gev_part* parts_b = PB.st[chr].parts[PB.cur];
    const size_t blk = std::min<size_t>(output_chunk(c, (size_t)1 << 30, 1), 4096), ba = std::min(blk, n_a), bb = std::min(blk, n_b);
    const size_t per_pair = (shared_bp ? 8 : 0) + (max_seg ? 8 : 0) + (n_seg ? 4 : 0);
    GEVC(c->ibd.out.ensure(ba * bb * per_pair, st));
    // the 8-byte matrices first: every part of the buffer begins on a multiple of its element
    u64* d_sh = shared_bp ? c->ibd.out.as<u64>() : nullptr;
    u64* d_mx = max_seg ? c->ibd.out.as<u64>() + (shared_bp ? ba * bb : 0) : nullptr;
    u32* d_ns = n_seg ? (u32*)(c->ibd.out.as<u64>() + ((shared_bp ? 1 : 0) + (max_seg ? 1 : 0)) * ba * bb) : nullptr;
    for (size_t ia = 0; ia < n_a; ia += blk)
        for (size_t ib = 0; ib < n_b; ib += blk) {
            const size_t na = std::min(blk, n_a - ia), nb = std::min(blk, n_b - ib);
            hipLaunchKernelGGL(k_ibd_tiles, dim3((unsigned)ceil_div(nb, GEV_IBD_TILE), (unsigned)ceil_div(na, GEV_IBD_TILE)), dim3(256), 0, st,
                               poff_a, parts_a, (u64)(a_begin + ia), (u32)na, poff_b, parts_b, (u64)(b_begin + ib), (u32)nb, (u64)min_bp, d_sh, d_ns, d_mx);
            KCHECK();
            const OptOut outs[3] = {{shared_bp, 8, na * nb, d_sh}, {max_seg, 8, na * nb, d_mx}, {n_seg, 4, na * nb, d_ns}};
            for (const OptOut& o : outs) if (o.host) GEVC(copy_out_block(c, o.host, o.el, n_b, ia, ib, na, nb, o.dev));
            HIPC(hipStreamSynchronize(st));
        }
    return GEV_OK;
}
int gev_ancestry_bp(gev_ctx* c, int pop, int chr, size_t row_begin, size_t n_rows, uint64_t* bp, uint32_t* n_parts)
{
    const char* who = "ancestry_bp";
    GEVC(ibd_begin(c, pop, chr, who));
    PopState& P = c->pop[pop];
    GEVC(check_range(who, "rows", row_begin, n_rows, 2 * P.n_people));
    if (!n_rows || (!bp && !n_parts)) return GEV_OK;
    if (n_rows > 0xffffffffull) return fail(GEV_EUNSUPPORTED, "%s: %zu rows in one call", who, n_rows);
    hipStream_t st = c->stream;
    const size_t npop = (size_t)c->n_pop;
    GEVC(c->ibd.out.ensure(n_rows * (8 * npop + 4), st));
    GEVC(c->ibd.flag.ensure(1, st));
    HIPC(hipMemsetAsync(c->ibd.flag.p, 0, sizeof(u32), st));
    u64* d_bp = c->ibd.out.as<u64>(); u32* d_np = (u32*)(d_bp + n_rows * npop);
    hipLaunchKernelGGL(k_ancestry_bp, dim3((unsigned)ceil_div(n_rows, 256)), dim3(256), 0, st, (const u32*)P.st[chr].poff[P.cur], (const gev_part*)P.st[chr].parts[P.cur],
                       (u64)row_begin, (u32)n_rows, c->n_pop, d_bp, d_np, c->ibd.flag.p);
    KCHECK();
    u32 flag = 0;
    HIPC(hipMemcpyAsync(&flag, c->ibd.flag.p, sizeof flag, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (flag) return fail(GEV_EINVAL, "%s: a part of population %d names a root population outside [0, %d)", who, pop, c->n_pop);
    const OptOut outs[2] = {{bp, sizeof(u64), n_rows * npop, d_bp}, {n_parts, sizeof(u32), n_rows, d_np}};
    return copy_back_outs(c, outs);
}
// what the host forms refuse of two sets of lists in host memory
static int ibd_host_lists(const char* who, const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b)
{
    if ((n_a && !off_a) || (n_b && !off_b)) return fail(GEV_EINVAL, "%s: null offsets", who);
    for (int side = 0; side < 2; side++) {
        const uint64_t* off = side ? off_b : off_a; const size_t n = side ? n_b : n_a;
        for (size_t r = 0; r < n; r++) {
            if (off[r + 1] < off[r]) return fail(GEV_EINVAL, "%s: the offsets of side %c decrease at row %zu", who, "ab"[side], r);
            if (off[r + 1] - off[r] > 0xffffffffull) return fail(GEV_EUNSUPPORTED, "%s: a row of %llu parts", who, (unsigned long long)(off[r + 1] - off[r]));
        }
        if (n && off[n] > off[0] && !(side ? parts_b : parts_a)) return fail(GEV_EINVAL, "%s: null parts", who);
    }
    return GEV_OK;
}
// the walk of gev_ibd.h compiled for the host on lists in host memory: no device, no context
int gev_dbg_ibd_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b,
                     uint64_t min_bp, uint64_t* shared_bp, uint32_t* n_seg, uint64_t* max_seg)
{
    GEVC(ibd_host_lists("dbg_ibd_host", parts_a, off_a, n_a, parts_b, off_b, n_b));
    gev_ibd_host(parts_a, off_a, n_a, parts_b, off_b, n_b, min_bp, shared_bp, n_seg, max_seg);
    return GEV_OK;
}
// ---- the IBD segments themselves (gev_ibd.h: k_ibd_segments) ----
// what the device and the host form refuse of the list's own arguments (pairs behind a null n_total, which list_args reports)
static int ibd_seg_args(const char* who, int pairs, const gev_ibd_segment* out, size_t capacity, const uint64_t* n_total)
{
    if (n_total && pairs != GEV_IBD_ALL_PAIRS && pairs != GEV_IBD_UPPER) return fail(GEV_EINVAL, "%s: pairs is %d (GEV_IBD_ALL_PAIRS or GEV_IBD_UPPER)", who, pairs);
    return list_args(who, out, capacity, n_total);
}
// one request's constants, and a strip of whole A rows [row0, +rows) of it against all its B rows
struct IbdSegCall { const u32 *poff_a, *poff_b; const gev_part *parts_a, *parts_b; size_t a_begin, b_begin, n_b; u64 min_bp; u32 upper; };
struct IbdStrip { size_t row0, rows; u64 total; };
static int ibd_seg_launch(gev_ctx* c, const IbdSegCall& q, size_t row0, size_t rows, bool fill)
{
    u32 ta_log2 = 0;
    while (ta_log2 < 4 && ((size_t)1 << ta_log2) < rows) ta_log2++;                          // the smallest tile height that holds the strip, 16 at the most
    const size_t tiles_b = ceil_div(q.n_b, (size_t)256 >> ta_log2), tiles = ceil_div(rows, (size_t)1 << ta_log2) * tiles_b;
    const auto kernel = fill ? k_ibd_segments<true> : k_ibd_segments<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(256), 0, c->stream, q.poff_a, q.parts_a, (u64)(q.a_begin + row0), (u32)rows,
                       q.poff_b, q.parts_b, (u64)q.b_begin, (u32)q.n_b, q.min_bp, q.upper, ta_log2, (u32)tiles_b,
                       fill ? c->list.off.p : c->list.cnt.p, c->ibd.seg.p);
    KCHECK();
    return GEV_OK;
}
// the strip's counts per pair into c->list.cnt; total: their sum in 64 bits, in host memory when this returns (null: not wanted)
static int ibd_seg_count(gev_ctx* c, const IbdSegCall& q, size_t row0, size_t rows, u64* total)
{
    hipStream_t st = c->stream;
    const size_t np = rows * q.n_b;
    GEVC(c->list.cnt.ensure(np, st));
    if (q.upper) HIPC(hipMemsetAsync(c->list.cnt.p, 0, np * sizeof(u32), st));             // (pairs on or below the diagonal are not visited)
    GEVC(ibd_seg_launch(c, q, row0, rows, false));
    return total ? count_total(c, c->list.cnt.p, np, total) : GEV_OK;
}
// Two phases.  Every strip is counted and its 64-bit total kept on the host: n_total.  If out holds them, each strip is counted again
// (a request of one strip still has its counts), scanned and filled into c->ibd.seg, which is copied to out at the running offset
// before the next strip's fill overwrites it.  Strips are whole A rows against all B rows, so row-major order inside a strip is the
// order of the list and strips concatenate.
int gev_ibd_segments(gev_ctx* c, int chr, int pop_a, size_t a_begin, size_t n_a, int pop_b, size_t b_begin, size_t n_b,
                     uint64_t min_bp, int pairs, gev_ibd_segment* out, size_t capacity, uint64_t* n_total)
{
    const char* who = "ibd_segments";
    GEVC(ibd_seg_args(who, pairs, out, capacity, n_total));
    GEVC(ibd_begin(c, pop_a, chr, who));
    if (pop_b != pop_a) GEVC(ibd_begin(c, pop_b, chr, who));
    PopState &PA = c->pop[pop_a], &PB = c->pop[pop_b];
    GEVC(check_range(who, "rows (a)", a_begin, n_a, 2 * PA.n_people));
    GEVC(check_range(who, "rows (b)", b_begin, n_b, 2 * PB.n_people));
    if (pairs == GEV_IBD_UPPER && pop_a != pop_b) return fail(GEV_EINVAL, "%s: GEV_IBD_UPPER takes one population (%d and %d given)", who, pop_a, pop_b);
    if (a_begin + n_a > ((size_t)1 << 32) || b_begin + n_b > ((size_t)1 << 32)) return fail(GEV_EUNSUPPORTED, "%s: rows beyond 2^32 - 1 do not fit a record", who);
    if (!n_a || !n_b) { *n_total = 0; return GEV_OK; }
    hipStream_t st = c->stream;
    const IbdSegCall q = {PA.st[chr].poff[PA.cur], PB.st[chr].poff[PB.cur], PA.st[chr].parts[PA.cur], PB.st[chr].parts[PB.cur], a_begin, b_begin, n_b, min_bp, pairs == GEV_IBD_UPPER ? 1u : 0u};
    const size_t strip_rows = std::min(output_chunk(c, (size_t)1 << 24, n_b), n_a);           // at most 2^24 pairs, at least one row
    const u64 budget = ((u64)1 << 30) / sizeof(gev_ibd_segment);                               // records of a strip on the device
    std::vector<IbdStrip> strips;
    u64 total = 0, largest = 0;
    for (size_t row0 = 0; row0 < n_a;) {
        size_t rows = std::min(strip_rows, n_a - row0);
        u64 t = 0;
        for (;;) {
            GEVC(ibd_seg_count(c, q, row0, rows, &t));
            if (t <= budget || rows == 1) break;
            rows /= 2;
        }
        if (t >> 32) return fail(GEV_EUNSUPPORTED, "%s: row %zu alone shares %llu segments with the %zu rows of side b", who, a_begin + row0, (unsigned long long)t, n_b);
        strips.push_back({row0, rows, t});
        total += t; largest = std::max(largest, t);
        row0 += rows;
    }
    *n_total = total;
    if (!total || total > capacity) return GEV_OK;
    GEVC(c->ibd.seg.ensure((size_t)largest, st));
    size_t done = 0;
    for (const IbdStrip& s : strips) {
        if (!s.total) continue;
        if (strips.size() > 1) GEVC(ibd_seg_count(c, q, s.row0, s.rows, nullptr));
        GEVC(fill_list(c, s.rows * n_b, s.total, c->ibd.seg, out + done, [&] { return ibd_seg_launch(c, q, s.row0, s.rows, true); }));
        done += (size_t)s.total;
    }
    return GEV_OK;
}
int gev_dbg_ibd_segments_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b,
                              uint64_t min_bp, int pairs, gev_ibd_segment* out, size_t capacity, uint64_t* n_total)
{
    const char* who = "dbg_ibd_segments_host";
    GEVC(ibd_seg_args(who, pairs, out, capacity, n_total));
    GEVC(ibd_host_lists(who, parts_a, off_a, n_a, parts_b, off_b, n_b));
    if (pairs == GEV_IBD_UPPER && (parts_a != parts_b || off_a != off_b)) return fail(GEV_EINVAL, "%s: GEV_IBD_UPPER takes the same lists on both sides", who);
    if (n_a > 0xffffffffull || n_b > 0xffffffffull) return fail(GEV_EUNSUPPORTED, "%s: rows beyond 2^32 - 1 do not fit a record", who);
    gev_ibd_segments_fit_host(parts_a, off_a, n_a, parts_b, off_b, n_b, min_bp, pairs == GEV_IBD_UPPER, out, capacity, n_total);
    return GEV_OK;
}
// ---- identity states per pair of individuals (gev_identity.h) -------------------------------------
// The pair matrix is walked in sub-blocks of at most 2048 individuals a side (gev_dbg_output_chunk caps them): a sub-block is one launch
// of k_identity_tiles into the nine planes of c->ibd.planes, each copied into its plane of the caller's before the next one's kernel runs.
int gev_identity_states(gev_ctx* c, int chr, int pop_a, size_t a_begin, size_t n_a, int pop_b, size_t b_begin, size_t n_b, uint64_t* bp)
{
    const char* who = "identity_states";
    GEVC(ibd_begin(c, pop_a, chr, who));
    if (pop_b != pop_a) GEVC(ibd_begin(c, pop_b, chr, who));
    PopState &PA = c->pop[pop_a], &PB = c->pop[pop_b];
    GEVC(check_range(who, "individuals (a)", a_begin, n_a, PA.n_people));
    GEVC(check_range(who, "individuals (b)", b_begin, n_b, PB.n_people));
    if (!n_a || !n_b) return GEV_OK;
    if (!bp) return fail(GEV_EINVAL, "%s: bp is null", who);
    hipStream_t st = c->stream;
    const u32* poff_a = PA.st[chr].poff[PA.cur]; const gev_part* parts_a = PA.st[chr].parts[PA.cur];
    const u32* poff_b = PB.st[chr].poff[PB.cur]; const gev_part* parts_b = PB.st[chr].parts[PB.cur];
    const size_t blk = std::min<size_t>(output_chunk(c, (size_t)1 << 30, 1), 2048), ba = std::min(blk, n_a), bb = std::min(blk, n_b);
    GEVC(c->ibd.planes.ensure(GEV_IDN_STATES * ba * bb, st));
    for (size_t ia = 0; ia < n_a; ia += blk)
        for (size_t ib = 0; ib < n_b; ib += blk) {
            const size_t na = std::min(blk, n_a - ia), nb = std::min(blk, n_b - ib);
            hipLaunchKernelGGL(k_identity_tiles, dim3((unsigned)ceil_div(nb, GEV_IDN_TILE), (unsigned)ceil_div(na, GEV_IDN_TILE)), dim3(256), 0, st,
                               poff_a, parts_a, (u64)(a_begin + ia), (u32)na, poff_b, parts_b, (u64)(b_begin + ib), (u32)nb, c->ibd.planes.p);
            KCHECK();
            for (size_t q = 0; q < GEV_IDN_STATES; q++) GEVC(copy_out_block(c, bp + q * n_a * n_b, sizeof(u64), n_b, ia, ib, na, nb, c->ibd.planes.p + q * na * nb));
            HIPC(hipStreamSynchronize(st));
        }
    return GEV_OK;
}
// the walk of gev_identity.h compiled for the host on lists in host memory: no device, no context
int gev_dbg_identity_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b, uint64_t* bp)
{
    const char* who = "dbg_identity_host";
    if (n_a > SIZE_MAX / 2 || n_b > SIZE_MAX / 2) return fail(GEV_EINVAL, "%s: %zu x %zu individuals", who, n_a, n_b);
    GEVC(ibd_host_lists(who, parts_a, off_a, 2 * n_a, parts_b, off_b, 2 * n_b));
    if (!n_a || !n_b) return GEV_OK;
    if (!bp) return fail(GEV_EINVAL, "%s: bp is null", who);
    gev_identity_host(parts_a, off_a, n_a, parts_b, off_b, n_b, bp);
    return GEV_OK;
}
// ---- founder lineages along the genome (gev_lineage.h) --------------------------------------------
// what the device calls and the host form refuse of the founder counts and the positions; tab: n_founder_haps[n_pop], then base[n_pop + 1]
static int lineage_args(const char* who, const uint64_t* pos, size_t n_pos, const uint64_t* n_founder_haps, int n_pop, std::vector<u64>& tab)
{
    if (!n_founder_haps) return fail(GEV_EINVAL, "%s: n_founder_haps is null", who);
    tab.assign(2 * (size_t)n_pop + 1, 0);
    u64 sum = 0;
    for (int q = 0; q < n_pop; q++) {
        if (n_founder_haps[q] > GEV_LINEAGE_MAX_F - sum) return fail(GEV_EUNSUPPORTED, "%s: more than 2^32 - 2 founder haplotypes in all", who);
        tab[q] = n_founder_haps[q]; tab[n_pop + q] = sum;
        sum += n_founder_haps[q];
    }
    tab[2 * (size_t)n_pop] = sum;
    if (n_pos && !pos) return fail(GEV_EINVAL, "%s: null positions", who);
    for (size_t i = 1; i < n_pos; i++)
        if (pos[i] < pos[i - 1]) return fail(GEV_EINVAL, "%s: the positions decrease at index %zu (%llu behind %llu)", who, i, (unsigned long long)pos[i], (unsigned long long)pos[i - 1]);
    return GEV_OK;
}
// what gev_lineage_check_row found
static int lineage_labels(const char* who, u32 bad, int n_pop)
{
    if (bad & GEV_LINEAGE_BAD_POP) return fail(GEV_EINVAL, "%s: a part names a root population outside [0, %d)", who, n_pop);
    if (bad & GEV_LINEAGE_BAD_HAP) return fail(GEV_EINVAL, "%s: a part's hap_index is at or beyond the founder haplotypes given for its root population", who);
    return GEV_OK;
}
// n_rows == 0: the per-position outputs of gev_founder_counts
static void lineage_no_rows(size_t n_pos, size_t F, int n_pop, uint32_t* counts, gev_lineage_site* site, uint32_t* pop_counts)
{
    if (counts) memset(counts, 0, n_pos * F * sizeof(u32));
    if (site) for (size_t p = 0; p < n_pos; p++) site[p] = gev_lineage_empty();
    if (pop_counts) memset(pop_counts, 0, n_pos * (size_t)n_pop * sizeof(u32));
}
// Both calls: at = gev_founder_at (fid alone).  The labels of all rows of the range are checked before anything leaves, so a call of
// several batches still writes nothing when it is refused.  A batch is the label kernel into c->lin.lab -- which is fid's own layout and
// leaves through copy_out_block -- or, for the counts, k_lineage_sites over it (and k_lineage_finish over its partials with several tiles).
static int lineage_run(gev_ctx* c, const char* who, bool at, int pop, int chr, size_t row_begin, size_t n_rows, const uint64_t* pos, size_t n_pos,
                       const uint64_t* n_founder_haps, uint32_t* fid, uint32_t* counts, gev_lineage_site* site, uint32_t* pop_counts)
{
    GEVC(ibd_begin(c, pop, chr, who));
    PopState& P = c->pop[pop];
    GEVC(check_range(who, "rows", row_begin, n_rows, 2 * P.n_people));
    std::vector<u64> tab;
    const int n_pop = c->n_pop;
    GEVC(lineage_args(who, pos, n_pos, n_founder_haps, n_pop, tab));
    const size_t F = (size_t)tab[2 * (size_t)n_pop];
    if (at && !fid && n_pos && n_rows) return fail(GEV_EINVAL, "%s: fid is null", who);
    if (n_rows > 0xffffffffull) return fail(GEV_EUNSUPPORTED, "%s: %zu rows in one call", who, n_rows);
    if (!n_pos) return GEV_OK;
    if (!n_rows) { if (!at) lineage_no_rows(n_pos, F, n_pop, counts, site, pop_counts); return GEV_OK; }
    hipStream_t st = c->stream;
    auto& S = c->lin;
    const u32* poff = P.st[chr].poff[P.cur]; const gev_part* parts = P.st[chr].parts[P.cur];
    GEVC(h2d(c, S.tab, tab.data(), tab.size()));
    GEVC(S.flag.ensure(1, st));
    HIPC(hipMemsetAsync(S.flag.p, 0, sizeof(u32), st));
    hipLaunchKernelGGL(k_lineage_check, dim3((unsigned)ceil_div(n_rows, 256)), dim3(256), 0, st, poff, parts, (u64)row_begin, (u32)n_rows, (const u64*)S.tab.p, n_pop, S.flag.p);
    KCHECK();
    u32 flag = 0;
    HIPC(hipMemcpyAsync(&flag, S.flag.p, sizeof flag, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    GEVC(lineage_labels(who, flag, n_pop));
    if (!at && !counts && !site && !pop_counts) return GEV_OK;
    GEVC(h2d(c, S.pos, pos, n_pos));
    const u64* d_base = S.tab.p + n_pop;
    const size_t n_tiles = std::max<size_t>(ceil_div(F, GEV_LINEAGE_TILE), 1);
    // a batch's positions: about 256 MB of labels and counts, and a grid of k_lineage_sites that fits 31 bits
    const size_t batch = std::min(std::min(output_chunk(c, 256u << 20, (n_rows + (counts ? F : 0)) * sizeof(u32)), n_pos), (size_t)0x7fffffff / n_tiles);
    GEVC(S.lab.ensure(batch * n_rows, st));
    if (!at) {
        GEVC(S.site.ensure(batch, st));
        GEVC(S.pop.ensure(batch * n_pop, st));
        if (counts) GEVC(S.counts.ensure(std::max<size_t>(batch * F, 1), st));
        if (n_tiles > 1) { GEVC(S.psite.ensure(batch * n_tiles, st)); GEVC(S.ppop.ensure(batch * n_tiles * n_pop, st)); }
    }
    for (size_t p0 = 0; p0 < n_pos; p0 += batch) {
        const size_t nb = std::min(batch, n_pos - p0);
        hipLaunchKernelGGL(k_lineage_labels, dim3((unsigned)ceil_div(n_rows, 256)), dim3(256), 0, st, poff, parts, (u64)row_begin, (u32)n_rows,
                           (const u64*)S.pos.p + p0, (u32)nb, d_base, S.lab.p);
        KCHECK();
        if (at) {
            GEVC(copy_out_block(c, fid, sizeof(u32), n_rows, p0, 0, nb, n_rows, S.lab.p));
            HIPC(hipStreamSynchronize(st));
            continue;
        }
        const bool one = n_tiles == 1;
        hipLaunchKernelGGL(k_lineage_sites, dim3((unsigned)(nb * n_tiles)), dim3(256), 0, st, (const u32*)S.lab.p, (u32)n_rows, d_base, n_pop, (u32)F, (u32)n_tiles,
                           counts ? S.counts.p : nullptr, one ? S.site.p : S.psite.p, one ? S.pop.p : S.ppop.p);
        if (!one) hipLaunchKernelGGL(k_lineage_finish, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, st, (const gev_lineage_site*)S.psite.p, (const u32*)S.ppop.p,
                                     (u32)nb, (u32)n_tiles, n_pop, S.site.p, S.pop.p);
        KCHECK();
        const OptOut outs[3] = {{site ? site + p0 : nullptr, sizeof(gev_lineage_site), nb, S.site.p}, {counts && F ? counts + p0 * F : nullptr, sizeof(u32), nb * F, S.counts.p},
                                {pop_counts ? pop_counts + p0 * n_pop : nullptr, sizeof(u32), nb * n_pop, S.pop.p}};
        GEVC(copy_back_outs(c, outs));
    }
    return GEV_OK;
}
int gev_founder_at(gev_ctx* c, int pop, int chr, size_t row_begin, size_t n_rows, const uint64_t* pos, size_t n_pos, const uint64_t* n_founder_haps, uint32_t* fid)
{
    return lineage_run(c, "founder_at", true, pop, chr, row_begin, n_rows, pos, n_pos, n_founder_haps, fid, nullptr, nullptr, nullptr);
}
int gev_founder_counts(gev_ctx* c, int pop, int chr, size_t row_begin, size_t n_rows, const uint64_t* pos, size_t n_pos, const uint64_t* n_founder_haps,
                       uint32_t* counts, gev_lineage_site* site, uint32_t* pop_counts)
{
    return lineage_run(c, "founder_counts", false, pop, chr, row_begin, n_rows, pos, n_pos, n_founder_haps, nullptr, counts, site, pop_counts);
}
// the walk and the reductions of gev_lineage.h compiled for the host on lists in host memory: no device, no context
int gev_dbg_lineage_host(const gev_part* parts, const uint64_t* off, size_t n_rows, const uint64_t* pos, size_t n_pos, const uint64_t* n_founder_haps, int n_pop,
                         uint32_t* fid, uint32_t* counts, gev_lineage_site* site, uint32_t* pop_counts)
{
    const char* who = "dbg_lineage_host";
    if (n_pop < 1) return fail(GEV_EINVAL, "%s: n_pop is %d", who, n_pop);
    GEVC(ibd_host_lists(who, parts, off, n_rows, nullptr, nullptr, 0));
    std::vector<u64> tab;
    GEVC(lineage_args(who, pos, n_pos, n_founder_haps, n_pop, tab));
    if (!n_pos) return GEV_OK;
    const size_t F = (size_t)tab[2 * (size_t)n_pop];
    if (!n_rows) { lineage_no_rows(n_pos, F, n_pop, counts, site, pop_counts); return GEV_OK; }
    u32 bad = 0;
    for (size_t r = 0; r < n_rows; r++) bad |= gev_lineage_check_row(parts + off[r], (uint32_t)(off[r + 1] - off[r]), tab.data(), n_pop);
    GEVC(lineage_labels(who, bad, n_pop));
    gev_lineage_host(parts, off, n_rows, pos, n_pos, tab.data() + n_pop, n_pop, fid, counts, site, pop_counts);
    return GEV_OK;
}
unsigned gev_dbg_lineage_tile(void) { return GEV_LINEAGE_TILE; }
// ---- runs of homozygosity (gev_roh.h) -------------------------------------------------------------
// what the device calls and the host form refuse of a request (params, the ranges, indices that do not fit a record's 32 bits)
static int roh_args(const char* who, const gev_roh_params* q, size_t snp_begin, size_t n_snps, size_t L, size_t ind_begin, size_t n_ind, size_t n_people)
{
    if (!q) return fail(GEV_EINVAL, "%s: params is null", who);
    GEVC(check_range(who, "SNPs", snp_begin, n_snps, L));
    GEVC(check_range(who, "individuals", ind_begin, n_ind, n_people));
    if (L >= 0xffffffffull || n_people > 0xffffffffull) return fail(GEV_EUNSUPPORTED, "%s: SNP or individual indices beyond 2^32 - 1 do not fit a record", who);
    return GEV_OK;
}
static int roh_begin(gev_ctx* c, int pop, int chr, const char* who, const gev_roh_params* q, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind)
{
    GEVC(output_begin(c, pop, chr, who, true));
    GEVC(ensure_csr(c, pop));
    return roh_args(who, q, snp_begin, n_snps, c->pop[pop].cs[chr].L, ind_begin, n_ind, c->pop[pop].n_people);
}
// the break bit plane of the chromosome into c->roh.brk (brk: null for max_gap_bp == 0, which has no breaks)
static int roh_breaks(gev_ctx* c, ChrStatic& S, u64 max_gap_bp, const uint4*& brk)
{
    brk = nullptr;
    if (!max_gap_bp) return GEV_OK;
    const size_t n_words = 2 * ceil_div(S.L, 128);
    GEVC(c->roh.brk.ensure(n_words, c->stream));
    hipLaunchKernelGGL(k_roh_breaks, dim3((unsigned)ceil_div(n_words, 256)), dim3(256), 0, c->stream, (const u64*)S.d_pos, (u64)S.L, max_gap_bp, (u32)n_words, c->roh.brk.p);
    KCHECK();
    brk = (const uint4*)c->roh.brk.p;
    return GEV_OK;
}
// one request's constants, and a scan of the n individuals staged from individual ind0 on
struct RohCall { const u64* pos; const uint4* brk; u32 chunks, snp_begin, n_snps; gev_roh_params q; };
static int roh_launch(gev_ctx* c, const RohCall& r, int mode, size_t ind0, size_t n, u32* n_roh, u64* roh_bp, u32* roh_snps, u64* max_bp, u32* diff, u32* cnt, gev_roh_segment* out)
{
    const auto kernel = mode == ROH_SUMMARY ? k_roh_scan<ROH_SUMMARY> : mode == ROH_COUNT ? k_roh_scan<ROH_COUNT> : k_roh_scan<ROH_FILL>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(n, ROH_WAVES)), dim3(ROH_WAVES * 64), 0, c->stream, (const uint4*)c->d_stage.as<uint4>(), r.chunks, (u32)n, (u32)ind0,
                       r.pos, r.brk, r.snp_begin, r.n_snps, r.q, n_roh, roh_bp, roh_snps, max_bp, diff, cnt, out);
    KCHECK();
    return GEV_OK;
}
// The individuals are staged in passes (ind_major_chunks); every pass's wave per individual writes entry i of the call's four vectors,
// the cover's difference array is the whole call's, scanned once behind the last pass.
int gev_roh_summary(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind, const gev_roh_params* q,
                    uint32_t* n_roh, uint64_t* roh_bp, uint32_t* roh_snps, uint64_t* max_bp, uint32_t* cover)
{
    const char* who = "roh_summary";
    GEVC(roh_begin(c, pop, chr, who, q, snp_begin, n_snps, ind_begin, n_ind));
    PopState& P = c->pop[pop]; ChrStatic& S = P.cs[chr];
    if (!n_ind) { if (cover && n_snps) memset(cover, 0, n_snps * sizeof(u32)); return GEV_OK; }
    OptOut outs[4] = {{n_roh, sizeof(u32), n_ind}, {roh_bp, sizeof(u64), n_ind}, {roh_snps, sizeof(u32), n_ind}, {max_bp, sizeof(u64), n_ind}};
    if (!n_snps) { zero_outs(outs); return GEV_OK; }
    if (!n_roh && !roh_bp && !roh_snps && !max_bp && !cover) return GEV_OK;
    hipStream_t st = c->stream;
    // the 8-byte vectors first: every part of the buffer begins on a multiple of its element
    GEVC(c->roh.out.ensure(n_ind * 24, st));
    u64* d_bp = c->roh.out.as<u64>(); u64* d_mx = d_bp + n_ind; u32* d_n = (u32*)(d_mx + n_ind); u32* d_sn = d_n + n_ind;
    outs[0].dev = d_n; outs[1].dev = d_bp; outs[2].dev = d_sn; outs[3].dev = d_mx;
    u32* d_diff = nullptr;
    if (cover) {
        GEVC(c->roh.diff.ensure(n_snps + 1, st));
        GEVC(c->roh.cov.ensure(n_snps + 1, st));
        d_diff = c->roh.diff.p;
        HIPC(hipMemsetAsync(d_diff, 0, (n_snps + 1) * sizeof(u32), st));
    }
    RohCall r = {S.d_pos, nullptr, (u32)(S.stride / 16), (u32)snp_begin, (u32)n_snps, *q};
    GEVC(roh_breaks(c, S, q->max_gap_bp, r.brk));
    GEVC(ind_major_chunks(c, pop, chr, ind_begin, n_ind, 2 * S.stride, [&](size_t i, size_t n) -> int {
        return roh_launch(c, r, ROH_SUMMARY, ind_begin + i, n, d_n + i, d_bp + i, d_sn + i, d_mx + i, d_diff, nullptr, nullptr);
    }));
    if (cover) {
        GEVC(scan_u32_on(st, c->d_sums, d_diff, n_snps, c->roh.cov.p));      // entry j + 1 = the inclusive sum up to j (mod 2^32, as the -1 entries are)
        HIPC(hipMemcpyAsync(cover, c->roh.cov.p + 1, n_snps * sizeof(u32), hipMemcpyDeviceToHost, st));
    }
    return copy_back_outs(c, outs);
}
// the counts of the staged pass into c->list.cnt (already large enough) and their 64-bit sum into *total (in host memory when this returns)
static int roh_count_pass(gev_ctx* c, const RohCall& r, size_t ind0, size_t n, u64* total)
{
    GEVC(roh_launch(c, r, ROH_COUNT, ind0, n, nullptr, nullptr, nullptr, nullptr, nullptr, c->list.cnt.p, nullptr));
    return count_total(c, c->list.cnt.p, n, total);
}
// the `total` records of the staged and counted pass into out (host) through c->roh.seg
static int roh_fill_pass(gev_ctx* c, const RohCall& r, size_t ind0, size_t n, u64 total, gev_roh_segment* out)
{
    if (total >> 32) return fail(GEV_EUNSUPPORTED, "roh_segments: %llu records in one pass", (unsigned long long)total);
    GEVC(c->roh.seg.ensure((size_t)total, c->stream));
    return fill_list(c, n, total, c->roh.seg, out, [&] { return roh_launch(c, r, ROH_FILL, ind0, n, nullptr, nullptr, nullptr, nullptr, nullptr, c->list.off.p, c->roh.seg.p); });
}
// A request of one pass counts, scans and fills on the same staged rows.  A request of several passes counts them all (n_total), and if
// out holds the records stages each again, counts it (the offsets of its fill) and fills: passes are runs of whole individuals in order,
// so their records concatenate.
int gev_roh_segments(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind, const gev_roh_params* q,
                     gev_roh_segment* out, size_t capacity, uint64_t* n_total)
{
    const char* who = "roh_segments";
    GEVC(list_args(who, out, capacity, n_total));
    GEVC(roh_begin(c, pop, chr, who, q, snp_begin, n_snps, ind_begin, n_ind));
    PopState& P = c->pop[pop]; ChrStatic& S = P.cs[chr];
    if (!n_ind || !n_snps) { *n_total = 0; return GEV_OK; }
    const size_t per_pass = std::min(output_chunk(c, 256u << 20, 2 * S.stride), n_ind);      // (what ind_major_chunks takes)
    const bool one_pass = per_pass == n_ind;
    GEVC(c->list.cnt.ensure(per_pass, c->stream));
    RohCall r = {S.d_pos, nullptr, (u32)(S.stride / 16), (u32)snp_begin, (u32)n_snps, *q};
    GEVC(roh_breaks(c, S, q->max_gap_bp, r.brk));
    u64 total = 0;
    GEVC(ind_major_chunks(c, pop, chr, ind_begin, n_ind, 2 * S.stride, [&](size_t i, size_t n) -> int {
        u64 t = 0;
        GEVC(roh_count_pass(c, r, ind_begin + i, n, &t));
        total += t;
        if (one_pass && t && t <= capacity) GEVC(roh_fill_pass(c, r, ind_begin + i, n, t, out));
        return GEV_OK;
    }));
    *n_total = total;
    if (one_pass || !total || total > capacity) return GEV_OK;
    size_t done = 0;
    return ind_major_chunks(c, pop, chr, ind_begin, n_ind, 2 * S.stride, [&](size_t i, size_t n) -> int {
        u64 t = 0;
        GEVC(roh_count_pass(c, r, ind_begin + i, n, &t));
        if (t) GEVC(roh_fill_pass(c, r, ind_begin + i, n, t, out + done));
        done += (size_t)t;
        return GEV_OK;
    });
}
// the walk of gev_roh.h compiled for the host on rows and positions in host memory: no device, no context
int gev_dbg_roh_host(const uint64_t* bits, size_t row_stride_words, size_t n_people, size_t L, const uint64_t* pos,
                     size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind, const gev_roh_params* q,
                     uint32_t* n_roh, uint64_t* roh_bp, uint32_t* roh_snps, uint64_t* max_bp, uint32_t* cover,
                     gev_roh_segment* out, size_t capacity, uint64_t* n_total)
{
    const char* who = "dbg_roh_host";
    if (n_total) GEVC(list_args(who, out, capacity, n_total));
    else if (out || capacity) return fail(GEV_EINVAL, "%s: an output list without n_total", who);
    GEVC(roh_args(who, q, snp_begin, n_snps, L, ind_begin, n_ind, n_people));
    if (n_snps && n_ind && (!bits || !pos || row_stride_words < ceil_div(L, 64))) return fail(GEV_EINVAL, "%s: null rows or positions, or rows of %zu words (%zu needed)", who, row_stride_words, ceil_div(L, 64));
    if (!n_ind) {
        if (cover && n_snps) memset(cover, 0, n_snps * sizeof(u32));
        if (n_total) *n_total = 0;
        return GEV_OK;
    }
    std::vector<u32> diff(cover ? n_snps + 1 : 0, 0);
    gev_roh_rows_host(bits, row_stride_words, pos, L, snp_begin, n_snps, ind_begin, n_ind, *q, n_roh, roh_bp, roh_snps, max_bp, cover ? diff.data() : nullptr, nullptr);
    if (cover) gev_roh_cover_host(diff.data(), n_snps, cover);
    if (n_total) gev_roh_segments_fit_host(bits, row_stride_words, pos, L, snp_begin, n_snps, ind_begin, n_ind, *q, out, capacity, n_total);
    return GEV_OK;
}
// ---- PLINK individual-major outputs ---------------------------------------------------------
// genotype columns of the PLINK .ped text, one line per individual (the caller writes the six id columns in front)
int gev_format_ped_text(gev_ctx* c, int pop, int chr, size_t ind_begin, size_t n_ind, const char* al0, const char* al1, char* out, size_t out_bytes)
{
    const char* who = "format_ped_text";
    GEVC(output_begin(c, pop, chr, who, true));
    ChrStatic& S = c->pop[pop].cs[chr];
    GEVC(check_range(who, "individuals", ind_begin, n_ind, c->pop[pop].n_people));
    const size_t line = 4 * S.L + 1;
    if ((al0 == nullptr) != (al1 == nullptr)) return fail(GEV_EINVAL, "format_ped_text: al0 and al1 must both be given or both be NULL");
    GEVC(check_out(who, out, n_ind, out_bytes, n_ind * line, "bytes"));
    hipStream_t st = c->stream;
    const char *d_al0 = nullptr, *d_al1 = nullptr;
    if (al0) {
        GEVC(c->d_tmp.ensure(std::max<size_t>(2 * S.L, 16), st));
        HIPC(hipMemcpyAsync(c->d_tmp.p, al0, S.L, hipMemcpyHostToDevice, st));
        HIPC(hipMemcpyAsync(c->d_tmp.as<char>() + S.L, al1, S.L, hipMemcpyHostToDevice, st));
        d_al0 = c->d_tmp.as<char>(); d_al1 = d_al0 + S.L;
    }
    return ind_major_chunks(c, pop, chr, ind_begin, n_ind, line, [&](size_t i, size_t n) -> int {
        return copy_out_text(c, n * line, out + i * line, [&] {
            hipLaunchKernelGGL(k_format_ped_text, dim3((unsigned)ceil_div(ceil_div(n * line, 16), 256)), dim3(256), 0, st, c->d_stage.as<u32>(), S.stride / 4, n, (u32)S.L, d_al0, d_al1, c->d_text.as<char>());
        });
    });
}
// matrix_plink_ped rows (bit 2*snp + hap), ceil(2L/64) words per individual
int gev_download_plink_matrix(gev_ctx* c, int pop, int chr, size_t ind_begin, size_t n_ind, u64* bits, size_t row_stride_words)
{
    const char* who = "download_plink_matrix";
    GEVC(output_begin(c, pop, chr, who, true));
    ChrStatic& S = c->pop[pop].cs[chr];
    GEVC(check_range(who, "individuals", ind_begin, n_ind, c->pop[pop].n_people));
    const size_t w32 = ceil_div(S.L, 32);                  // one source word -> one 64-bit output word
    GEVC(check_out(who, bits, n_ind, row_stride_words, w32, "words per row"));
    return ind_major_chunks(c, pop, chr, ind_begin, n_ind, w32 * 8, [&](size_t i, size_t n) -> int {
        GEVC(c->d_text.ensure(std::max<size_t>(n * w32 * 8, 16), c->stream));
        if (w32) hipLaunchKernelGGL(k_interleave_haps, dim3((unsigned)ceil_div(n * w32, 256)), dim3(256), 0, c->stream, c->d_stage.as<u32>(), S.stride / 4, n, (u32)w32, c->d_text.as<u64>(), w32);
        KCHECK();
        return copy_out_rows(c, c->d_text.p, w32 * 8, w32 * 8, n, bits + i * row_stride_words, row_stride_words);
    });
}
// ---- K8: tiles of the genotype matrix from the interval state and founder tiles -------------------
// rows [row_begin, +n_rows) x loci [snp_begin, +n_snps); one founder tile per root population (after migration a part may descend
// from another population's founders, :1204)
static int materialize_begin(gev_ctx* c, int pop, int chr, size_t row_begin, size_t n_rows, size_t snp_begin, size_t n_snps)
{
    GEVC(output_begin(c, pop, chr, "materialize", false));
    if (!c->track_intervals) return fail(GEV_ESTATE, "materialize: interval tracking is disabled");
    GEVC(check_range("materialize", "rows", row_begin, n_rows, 2 * c->pop[pop].n_people));
    return check_range("materialize", "SNPs", snp_begin, n_snps, c->pop[pop].cs[chr].L);
}
// founder tiles to the device (c->d_snpmajor, stacked population after population; row offsets in c->d_map)
static int upload_founder_tiles(gev_ctx* c, size_t n_snps, const u64* const* founder_bits, const size_t* founder_stride_words, const size_t* n_founder_rows)
{
    const size_t w64 = ceil_div(n_snps, 64);
    if (!founder_bits || !founder_stride_words || !n_founder_rows) return fail(GEV_EINVAL, "materialize: bad founder tile");
    std::vector<u64> row0(c->n_pop + 1, 0);
    for (int p = 0; p < c->n_pop; p++) {
        if (n_founder_rows[p] && (!founder_bits[p] || founder_stride_words[p] < w64)) return fail(GEV_EINVAL, "materialize: bad founder tile of population %d", p);
        row0[p + 1] = row0[p] + n_founder_rows[p];
    }
    if (!row0[c->n_pop]) return fail(GEV_EINVAL, "materialize: bad founder tile");
    hipStream_t st = c->stream;
    GEVC(c->d_snpmajor.ensure(row0[c->n_pop] * w64 * 8, st));
    for (int p = 0; p < c->n_pop; p++)
        if (n_founder_rows[p])
            HIPC(hipMemcpy2DAsync(c->d_snpmajor.as<u64>() + row0[p] * w64, w64 * 8, founder_bits[p], founder_stride_words[p] * 8, w64 * 8, n_founder_rows[p], hipMemcpyHostToDevice, st));
    GEVC(c->d_map.ensure((c->n_pop + 1) * sizeof(u64) + 16, st));
    HIPC(hipMemcpyAsync(c->d_map.p, row0.data(), (c->n_pop + 1) * sizeof(u64), hipMemcpyHostToDevice, st));
    HIPC(hipStreamSynchronize(st));                      // row0 is a local
    GEVC(c->d_flag.ensure(16, st));
    HIPC(hipMemsetAsync(c->d_flag.p, 0, 4, st));
    return GEV_OK;
}
// rows [row0, row0+nr) of the tile into `out` (nr x w64 words, mutations applied); `plain` = scratch of the same size
static int materialize_rows(gev_ctx* c, int pop, int chr, size_t row0, size_t nr, size_t snp_begin, size_t n_snps, u64* plain, u64* out)
{
    PopState& P = c->pop[pop]; ChrStatic& S = P.cs[chr]; ChrState& cs = P.st[chr];
    hipStream_t st = c->stream;
    const size_t w64 = ceil_div(n_snps, 64), w32 = 2 * w64;
    GEVC(ensure_csr(c, pop));
    HIPC(hipMemsetAsync(plain, 0, nr * w64 * 8, st));                                     // pad bits of the last word stay 0
    hipLaunchKernelGGL(k_materialize_tile, dim3((unsigned)ceil_div(nr * ceil_div(n_snps, 32), 256)), dim3(256), 0, st,
                       cs.poff[P.cur], cs.parts[P.cur], row0, nr, S.d_pos, (u32)snp_begin, (u32)n_snps,
                       c->d_snpmajor.as<u32>(), w32, c->d_map.as<u64>(), c->n_pop, (u32*)plain, w32, c->d_flag.as<u32>());
    HIPC(hipMemcpyAsync(out, plain, nr * w64 * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_tile_apply_mut, dim3((unsigned)ceil_div(nr, 256)), dim3(256), 0, st, (const u32*)plain, (u32*)out, w32, row0, nr,
                       cs.moff[P.cur], cs.mpos[P.cur], S.d_pos, (u32)snp_begin, (u32)n_snps);
    KCHECK();
    return GEV_OK;
}
static int materialize_status(gev_ctx* c)
{
    u32 flag = 0;
    HIPC(hipMemcpy(&flag, c->d_flag.p, 4, hipMemcpyDeviceToHost));
    if (flag) return fail(GEV_EINVAL, "materialize: Error: p.hap_index is not in range");
    return GEV_OK;
}
int gev_materialize_pops(gev_ctx* c, int pop, int chr, size_t row_begin, size_t n_rows, size_t snp_begin, size_t n_snps,
                         const u64* const* founder_bits, const size_t* founder_stride_words, const size_t* n_founder_rows, u64* bits, size_t row_stride_words)
{
    GEVC(materialize_begin(c, pop, chr, row_begin, n_rows, snp_begin, n_snps));
    if (!n_rows || !n_snps) return GEV_OK;
    GEVC(upload_founder_tiles(c, n_snps, founder_bits, founder_stride_words, n_founder_rows));
    const size_t w64 = ceil_div(n_snps, 64);
    GEVC(check_out("materialize", bits, n_rows, row_stride_words, w64, "words per row"));
    hipStream_t st = c->stream;
    const size_t max_rows = output_chunk(c, 128u << 20, w64 * 8);
    for (size_t r0 = 0; r0 < n_rows; r0 += max_rows) {
        const size_t nr = std::min(max_rows, n_rows - r0);
        GEVC(c->d_stage.ensure(nr * w64 * 8, st)); GEVC(c->d_text.ensure(nr * w64 * 8, st));
        GEVC(materialize_rows(c, pop, chr, row_begin + r0, nr, snp_begin, n_snps, c->d_stage.as<u64>(), c->d_text.as<u64>()));
        GEVC(copy_out_rows(c, c->d_text.p, w64 * 8, w64 * 8, nr, bits + r0 * row_stride_words, row_stride_words));
    }
    return materialize_status(c);
}
// PLINK .bed body of SNPs [snp_begin, +n_snps) straight from the interval state (BASELINE config 5: "PLINK bit-packed output" of a
// population whose genotype matrix is never resident): tile of ALL haplotype rows -> 64x64 bit-tile transpose -> 2-bit packing
int gev_materialize_bed(gev_ctx* c, int pop, int chr, size_t snp_begin, size_t n_snps,
                        const u64* const* founder_bits, const size_t* founder_stride_words, const size_t* n_founder_rows, uint8_t* out, size_t out_bytes)
{
    GEVC(materialize_begin(c, pop, chr, 0, 0, snp_begin, n_snps));
    PopState& P = c->pop[pop];
    const size_t rows = 2 * P.n_people, bpl = ceil_div(P.n_people, 4), w64 = ceil_div(n_snps, 64);
    if (!n_snps || !rows) return GEV_OK;
    GEVC(upload_founder_tiles(c, n_snps, founder_bits, founder_stride_words, n_founder_rows));
    GEVC(check_out("materialize_bed", out, n_snps, out_bytes, n_snps * bpl, "bytes"));
    hipStream_t st = c->stream;
    GEVC(c->d_stage.ensure(rows * w64 * 8, st)); GEVC(c->d_tmp.ensure(rows * w64 * 8, st));
    GEVC(materialize_rows(c, pop, chr, 0, rows, snp_begin, n_snps, c->d_stage.as<u64>(), c->d_tmp.as<u64>()));
    const size_t stride_sm = ceil_div(rows, 64);
    GEVC(c->d_text.ensure(std::max<size_t>(n_snps * stride_sm * 8 + n_snps * bpl, 16), st));
    u64* snpmajor = c->d_text.as<u64>(); uint8_t* bed = c->d_text.as<uint8_t>() + n_snps * stride_sm * 8;
    HIPC(hipMemsetAsync(snpmajor, 0, n_snps * stride_sm * 8, st));
    const u32 wpw = 16;
    hipLaunchKernelGGL(k_transpose_tiles, dim3((unsigned)stride_sm, (unsigned)ceil_div(ceil_div(w64, wpw), 4)), dim3(256), 0, st, c->d_tmp.as<u64>(), RowMap{}, w64, rows, (u32)n_snps,
                       0u, (u32)n_snps, snpmajor, stride_sm, wpw);
    hipLaunchKernelGGL(k_format_bed, dim3((unsigned)ceil_div(n_snps * bpl, 256)), dim3(256), 0, st, snpmajor, stride_sm, P.n_people, (u32)n_snps, bed);
    KCHECK();
    HIPC(hipMemcpyAsync(out, bed, n_snps * bpl, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return materialize_status(c);
}
// one population per context: a single founder tile
int gev_materialize(gev_ctx* c, int pop, int chr, size_t row_begin, size_t n_rows, size_t snp_begin, size_t n_snps,
                    const u64* founder_bits, size_t founder_stride_words, size_t n_founder_rows, u64* bits, size_t row_stride_words)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (c->n_pop > 1) return fail(GEV_EINVAL, "materialize: this context has %d populations: use gev_materialize_pops (one founder tile per root population)", c->n_pop);
    return gev_materialize_pops(c, pop, chr, row_begin, n_rows, snp_begin, n_snps, &founder_bits, &founder_stride_words, &n_founder_rows, bits, row_stride_words);
}

int gev_download_cv(gev_ctx* c, int pop, int phen, int chr, u64* bits, size_t row_stride_words)
{
    GEVC(check_idx(c, pop, chr, phen));
    GEVC(check_active(c, chr, "download_cv"));
    PopState& P = c->pop[pop]; CvStatic& V = P.cv[phen][chr];
    if (!P.gen0) return fail(GEV_ESTATE, "download_cv: population %d has no current generation", pop);
    GEVC(materialize_order(c, pop));
    if (!bits || row_stride_words * 64 < V.C) return fail(GEV_EINVAL, "download_cv: bad output buffer");
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t rows = 2 * P.n_people;
    GEVC(c->d_cvm.ensure(std::max<size_t>(rows * V.sub_w32, 4), st));
    GEVC(c->d_tmp.ensure(rows * row_stride_words * 8, st));
    hipLaunchKernelGGL(k_cv_resolve, dim3((unsigned)ceil_div(rows * V.sub_w32, 256)), dim3(256), 0, st,
                       P.cvp[phen][chr][P.cur], V.stride_w32, V.sub_w32, c->d_cvm, rows);
    HIPC(hipMemsetAsync(c->d_tmp.p, 0, rows * row_stride_words * 8, st));
    if (V.C)
        hipLaunchKernelGGL(k_permute_cols, dim3((unsigned)ceil_div(rows * V.sub_w32, 256)), dim3(256), 0, st,
                           c->d_cvm, (size_t)V.sub_w32, c->d_tmp.as<u32>(), row_stride_words * 2, V.sub_w32, V.d_col_of_icv, V.C, rows);
    KCHECK();
    HIPC(hipMemcpyAsync(bits, c->d_tmp.p, rows * row_stride_words * 8, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
int gev_download_intervals(gev_ctx* c, int pop, int chr, gev_part* out, u64* hap_offsets, size_t* n_parts)
{
    GEVC(output_begin(c, pop, chr, "download_intervals", false));
    GEVC(ensure_csr(c, pop));
    if (!c->track_intervals) return fail(GEV_ESTATE, "download_intervals: interval tracking is disabled");
    PopState& P = c->pop[pop]; ChrState& cs = P.st[chr];
    return download_list(c, pop, "download_intervals", cs.poff[P.cur], cs.parts[P.cur], out, hap_offsets, n_parts);
}
int gev_download_mutations(gev_ctx* c, int pop, int chr, u64* out, u64* hap_offsets, size_t* n_mut)
{
    GEVC(output_begin(c, pop, chr, "download_mutations", false));
    GEVC(ensure_csr(c, pop));
    PopState& P = c->pop[pop]; ChrState& cs = P.st[chr];
    return download_list(c, pop, "download_mutations", cs.moff[P.cur], cs.mpos[P.cur], out, hap_offsets, n_mut);
}

// ---- introspection ------------------------------------------------------------------------
int gev_pop_size(gev_ctx* c, int pop, size_t* n)          // (the published generation's size; allowed while a generation is in flight)
{
    if (!c || !n) return fail(GEV_EINVAL, "null");
    if (pop < 0 || pop >= c->n_pop) return fail(GEV_EINVAL, "population index %d out of range", pop);
    *n = c->pop[pop].n_people;
    return GEV_OK;
}
int gev_plane_ptr(gev_ctx* c, int pop, int chr, void** dptr, size_t* unit_bytes, size_t* n_slots, const uint32_t** unit_of, uint32_t* segments_per_row)
{
    if (c) GEVC(check_dense(c, "plane_ptr"));
    GEVC(check_idx(c, pop, chr));
    GEVC(check_active(c, chr, "plane_ptr"));
    GEVC(gev_sync(c));
    if (c->pop[pop].gen0) GEVC(materialize_order(c, pop));
    PopState& P = c->pop[pop];
    if (dptr) *dptr = P.st[chr].pool.p;
    if (unit_of) *unit_of = P.st[chr].phys[P.pcur];
    if (unit_bytes) *unit_bytes = P.cs[chr].unit_bytes();
    if (segments_per_row) *segments_per_row = P.cs[chr].nseg;
    if (n_slots) *n_slots = 2 * P.n_people;
    return GEV_OK;
}
int gev_stream(gev_ctx* c, void** s) { if (!c || !s) return fail(GEV_EINVAL, "null"); *s = (void*)c->stream; return GEV_OK; }
int gev_last_reproduce_ms(gev_ctx* c, float ms[4]) { if (!c || !ms) return fail(GEV_EINVAL, "null"); GEVC(gev_sync(c)); for (int i = 0; i < 4; i++) ms[i] = c->last_ms[i]; return GEV_OK; }
// ---- Simulation::ras_scale_AD_compute_GEF for every phenotype, fed from the device (gev_phenotypes.h) ------------------------------
static int ph_enqueue(gev_ctx* c)
{
    gev_ctx::PhenoState& H = c->ph;
    PopState& P = c->pop[H.pop];
    hipStream_t st = c->stream;
    const size_t n = P.n_people; const int nphen = c->nphen; const bool gen0 = H.gen_num == 0;
    int nvc = 0;
    for (int p = 0; p < nphen; p++) nvc += H.scheme[p].vc > 0;
    const size_t n_seeds = (gen0 ? nvc : 0) + nphen;
    H.n = n; H.n_seeds = n_seeds; H.words = round_up(PHR_SEEDS + n_seeds, 2);
    const size_t n_stats = (size_t)nphen * (1 + PH_COMP + 2);                  // {mean, var}: e, 7 components, raw A, raw D per phenotype
    const size_t res_bytes = H.words * sizeof(u32) + n_stats * 2 * sizeof(double);
    GEVC(H.res.ensure(res_bytes, st)); GEVC(H.starts.ensure((nphen + 2), st));
    HIPC(hipMemsetAsync(H.res.p, 0, res_bytes, st)); HIPC(hipMemsetAsync(H.starts.p, 0, (nphen + 2) * sizeof(u32), st));
    u32* res = H.res.as<u32>(); u32* seeds = res + PHR_SEEDS;
    double* e_stats = (double*)(res + H.words); double* comp_stats = e_stats + 2 * nphen; double* a_stats = comp_stats + 2 * nphen * PH_COMP; double* d_stats = a_stats + 2 * nphen;
    // the ras_glob_seed() values: generation 0 one per phenotype with vc > 0 (:3058), then one per phenotype (:3078)
    GEVC(enqueue_glob(H.globblk, st, H.glob_state, nullptr, n_seeds, seeds, res + PHR_STATE, res + PHR_FLAGS));
    Dev<double>& comp = P.d_comp[P.cbuf];
    GEVC(comp.ensure((size_t)nphen * PH_COMP * n, st));
    GEVC(H.eraw.ensure((size_t)nphen * n, st));
    const size_t cval_stride = gen0 ? 1 : std::max<size_t>(P.cs_ncouples, 1);
    if (!gen0 && nvc) GEVC(H.cval.ensure((size_t)nphen * cval_stride, st));
    // _var_a_gen0 / _var_d_gen0 (:557-561) from the raw A/D; the host needs them for s_a / s_d: generation 0 waits once for them
    if (gen0 && !P.ad0_ok) {
        GEVC(ph_var(c, c->d_add, 1, (size_t)nphen, n, (unsigned)nphen, a_stats));
        GEVC(ph_var(c, c->d_dom, 1, (size_t)nphen, n, (unsigned)nphen, d_stats));
        std::vector<double> h(4 * (size_t)nphen);
        HIPC(hipMemcpyAsync(h.data(), a_stats, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        P.ad0.assign(2 * (size_t)nphen, 0.0);
        for (int p = 0; p < nphen; p++) { P.ad0[2 * p] = h[2 * p + 1]; P.ad0[2 * p + 1] = h[2 * nphen + 2 * p + 1]; }
        P.ad0_ok = true;
    }
    // the normal streams.  Independent ones in one batch: the noise of every phenotype (:3080-3102), generation 0's family effect
    // (an engine of its own seed per phenotype, :3053-3066) and parental effect (generator_f(seed + 1), :3095-3114)
    std::vector<NrmStream> batch;
    std::vector<PhTask> tasks(nphen);
    int kvc = 0;
    for (int p = 0; p < nphen; p++) {
        const gev_pheno_scheme& S = H.scheme[p];
        double* o = comp + (size_t)p * PH_COMP * n;
        NrmStream e{}; e.seed_idx = (int)(gen0 ? nvc : 0) + p; e.start_idx = e.next_idx = -1; e.n = n; e.n_cand = ph_candidates(c, n, H.cand_shift); e.sd = 1.0; e.out = H.eraw + (size_t)p * n;
        batch.push_back(e);
        if (gen0 && S.vc > 0) { NrmStream s = e; s.seed_idx = kvc++; s.sd = std::sqrt(S.vc); s.out = o + PH_C * n; batch.push_back(s); }
        if (gen0 && S.vf > 0) { NrmStream s = e; s.seed_add = 1; s.sd = std::sqrt(S.vf); s.out = o + PH_F * n; batch.push_back(s); }
        PhTask& t = tasks[p];
        t.s_a = 1; if (S.va > 0) t.s_a = std::sqrt(P.ad0[2 * p] / S.va);
        t.s_d = 0; if (S.vd > 0) t.s_d = std::sqrt(P.ad0[2 * p + 1] / S.vd); else if (S.vd == -1) t.s_d = 1;
        t.ve = S.ve; t.vf = S.vf; t.beta = S.beta;
        t.has_c = S.vc > 0; t.c_by_couple = !gen0; t.f_gather = !gen0;
        t.prev_plane = H.vt_type == 1 ? 0 : (H.vt_type == 2 ? 1 : -1);
    }
    // reproduce's family effect (:2417-2429): ONE engine (seed_reproduce + 1), a fresh distribution per phenotype with vc > 0 -- each
    // starts at the candidate pair behind the last one its predecessor consumed, a device word.  The first one starts at pair 0 and
    // rides with the batch; every later one is a launch pair of its own behind its predecessor
    std::vector<std::vector<NrmStream>> chained;
    if (!gen0) {
        int k = 0;
        for (int p = 0; p < nphen; p++) {
            if (!(H.scheme[p].vc > 0)) continue;
            NrmStream s{}; s.seed_idx = -1; s.seed_val = P.cs_seed; s.seed_add = 1; s.start_idx = k; s.next_idx = k + 1; s.n = P.cs_ncouples; s.n_cand = ph_candidates(c, P.cs_ncouples, H.cand_shift);
            s.sd = std::sqrt(H.scheme[p].vc); s.out = H.cval + (size_t)p * cval_stride;
            if (k == 0) batch.push_back(s); else chained.push_back(std::vector<NrmStream>(1, s));
            k++;
        }
    }
    GEVC(ph_streams(c, batch, seeds, H.starts, res + PHR_FLAGS));
    for (auto& one : chained) GEVC(ph_streams(c, one, seeds, H.starts, res + PHR_FLAGS));
    GEVC(ph_var(c, H.eraw, n, 1, n, (unsigned)nphen, e_stats));                       // CommFunc::var(e), two passes, n-1
    GEVC(upload_table(c, H.tasks, tasks.data(), tasks.size(), st));
    Dev<double>& keep = P.d_phen[P.sbuf];
    GEVC(keep.ensure(n * (size_t)nphen, st));
    hipLaunchKernelGGL(k_ph_apply, dim3((unsigned)ceil_div(n, 256), (unsigned)nphen), dim3(256), 0, st, H.tasks, c->d_add,
                       c->d_dom, n, (u32)nphen, H.eraw, (const double*)e_stats, H.cval, cval_stride,
                       P.d_ids[P.ibuf], P.ids_stride[P.ibuf], P.d_cidx[P.ibuf],
                       P.d_prev, P.prev_n, comp, keep, res);
    KCHECK();
    GEVC(ph_var(c, comp, n, 1, n, (unsigned)nphen * PH_COMP, comp_stats));           // CommFunc::var of A D G C E F P (:2023-2037)
    GEVC(H.h_res.ensure(res_bytes, res_bytes * 2 + 256, st));
    HIPC(hipMemcpyAsync(H.h_res.p, H.res.p, res_bytes, hipMemcpyDeviceToHost, st));
    if (!H.ev) GEVC(H.ev.create(hipEventDisableTiming));
    HIPC(hipEventRecord(H.ev, st));
    return GEV_OK;
}
int gev_generation_phenotypes(gev_ctx* c, int pop, const gev_phenotypes_params* par, uint32_t glob_state)
{
    GEVC(check_idx(c, pop, 0));
    if (!par || !par->scheme) return fail(GEV_EINVAL, "generation_phenotypes: null parameters");
    if (par->gen_num < 0) return fail(GEV_EINVAL, "generation_phenotypes: gen_num %d", par->gen_num);
    if (glob_state == 0 || glob_state >= GEV_M31) return fail(GEV_EINVAL, "generation_phenotypes: %u is not a state of std::minstd_rand0 (1 .. 2^31-2)", glob_state);
    if (!c->track_pedigree) return fail(GEV_ESTATE, "generation_phenotypes: the context does not track pedigree ids (gev_set_track_pedigree)");
    if (c->any_inactive && c->ad_host_set_pop != pop)
        return fail(GEV_ESTATE, "generation_phenotypes: this context holds a subset of the chromosomes: give it the all-reduced raw A/D first (gev_set_ad / gev_ad_finish_device)");
    PopState& P = c->pop[pop];
    if (!P.gen0) return fail(GEV_ESTATE, "generation_phenotypes: population %d has no current generation", pop);
    const bool gen0 = par->gen_num == 0;
    bool any_vc = false, any_vf = false;
    for (int p = 0; p < c->nphen; p++) { any_vc |= par->scheme[p].vc > 0; any_vf |= par->scheme[p].vf > 0; }
    if (!P.ids_ok) return fail(GEV_ESTATE, "generation_phenotypes: population %d's pedigree ids were dropped when its rows changed (gev_upload_pedigree restores them)", pop);
    if (!gen0 && !P.ad0_ok) return fail(GEV_ESTATE, "generation_phenotypes: population %d has no generation-0 variances of A and D (gen_num 0 first, or gev_set_ad_gen0)", pop);
    if (!gen0 && any_vf && (par->vt_type == 1 || par->vt_type == 2) && !P.prev_ok)
        return fail(GEV_ESTATE, "generation_phenotypes: vf > 0 at generation %d needs the saved record of the generation before (gev_save_prev_gen / gev_upload_prev_gen)", par->gen_num);
    HIPC(hipSetDevice(c->device));
    GEVC(materialize_order(c, pop));
    if (!gen0 && any_vc && !P.cs_ok)
        return fail(GEV_ESTATE, "generation_phenotypes: population %d's rows changed since its generation was published: the family effects of its couples can no longer be handed out", pop);
    if (c->ad_cached_pop != pop && c->ad_host_set_pop != pop) GEVC(gev_compute_ad(c, pop, nullptr, nullptr, nullptr, nullptr));      // raw A/D of this generation on the device
    gev_ctx::PhenoState& H = c->ph;
    if (H.pending && c->pop[H.pop].layout_epoch == H.epoch)
        return fail(GEV_ESTATE, "generation_phenotypes: the step of population %d is outstanding: call gev_phenotypes_result first", H.pop);
    H.pop = pop; H.gen_num = par->gen_num; H.vt_type = par->vt_type; H.glob_state = glob_state; H.epoch = P.layout_epoch;
    H.scheme.assign(par->scheme, par->scheme + c->nphen);
    H.pending = false;
    if (H.short_candidates) H.cand_shift = 0;                // (test hook: every step starts too short)
    GEVC(ph_enqueue(c));
    H.pending = true;
    P.comp_ok = true; std::fill(P.phen_ok.begin(), P.phen_ok.end(), 1);
    return GEV_OK;
}
int gev_phenotypes_result(gev_ctx* c, int pop, uint32_t* glob_state_after, uint32_t* seeds, double* var)
{
    GEVC(check_idx(c, pop, 0));
    gev_ctx::PhenoState& H = c->ph;
    if (!H.pending || H.pop != pop) return fail(GEV_ESTATE, "phenotypes_result: no gev_generation_phenotypes of population %d is outstanding", pop);
    PopState& P = c->pop[pop];
    if (H.epoch != P.layout_epoch) { H.pending = false; return fail(GEV_ESTATE, "phenotypes_result: population %d changed since gev_generation_phenotypes", pop); }
    HIPC(hipSetDevice(c->device));
    for (int attempt = 0;; attempt++) {
        HIPC(hipEventSynchronize(H.ev));
        const u32* w = (const u32*)H.h_res.p;
        const u32 flags = w[PHR_FLAGS];
        if (flags & FLAG_RNG_SHORT) { H.pending = false; P.comp_ok = false; P.drop_selection(); return fail(GEV_EDEVICE, "generation_phenotypes: the seed stream ran out of candidates (internal error)"); }
        if (flags & PHF_CAND_SHORT) {                        // acceptance far below pi/4 (or the test hook): the step again with more candidate pairs
            if (attempt == 6) { H.pending = false; P.comp_ok = false; P.drop_selection(); return fail(GEV_EDEVICE, "generation_phenotypes: normal streams still short of candidates after %d attempts", attempt + 1); }
            H.cand_shift++; H.reruns++;
            P.sel_ok = false;                                // (selection values computed meanwhile came from the short streams)
            GEVC(ph_enqueue(c));
            continue;
        }
        H.pending = false;
        if (flags & PHF_ID_RANGE) {
            P.comp_ok = false; P.drop_selection();
            return fail(GEV_EUNSUPPORTED, "generation_phenotypes: %u individuals of population %d have a parent id at or beyond the %zu entries of the saved record "
                        "(the reference reads past the end of its array there)", w[PHR_NBAD], pop, P.prev_n);
        }
        if (glob_state_after) *glob_state_after = w[PHR_STATE];
        if (seeds) memcpy(seeds, w + PHR_SEEDS, H.n_seeds * sizeof(u32));
        if (var) {
            const double* cs = (const double*)(w + H.words) + 2 * c->nphen;
            for (int k = 0; k < c->nphen * PH_COMP; k++) var[k] = cs[2 * k + 1];
        }
        return GEV_OK;
    }
}
int gev_download_phenotypes(gev_ctx* c, int pop, int phen, double* out)
{
    GEVC(check_idx(c, pop, 0, phen));
    if (!out) return fail(GEV_EINVAL, "download_phenotypes: null output");
    PopState& P = c->pop[pop];
    if (!P.gen0 || !P.comp_ok) return fail(GEV_ESTATE, "download_phenotypes: population %d has no phenotype components of its current individuals (gev_generation_phenotypes)", pop);
    HIPC(hipSetDevice(c->device));
    const size_t n = P.n_people;
    HIPC(hipMemcpyAsync(out, P.d_comp[P.cbuf] + (size_t)phen * PH_COMP * n, PH_COMP * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return GEV_OK;
}
int gev_get_ad_gen0(gev_ctx* c, int pop, int phen, double* var_a, double* var_d)
{
    GEVC(check_idx(c, pop, 0, phen));
    PopState& P = c->pop[pop];
    if (!P.ad0_ok) return fail(GEV_ESTATE, "get_ad_gen0: population %d has no generation-0 variances of A and D", pop);
    if (var_a) *var_a = P.ad0[2 * phen];
    if (var_d) *var_d = P.ad0[2 * phen + 1];
    return GEV_OK;
}
int gev_set_ad_gen0(gev_ctx* c, int pop, int phen, double var_a, double var_d)
{
    GEVC(check_idx(c, pop, 0, phen));
    PopState& P = c->pop[pop];
    if (P.ad0.size() != 2 * (size_t)c->nphen) P.ad0.assign(2 * (size_t)c->nphen, 0.0);
    P.ad0[2 * phen] = var_a; P.ad0[2 * phen + 1] = var_d;
    P.ad0_ok = true;
    return GEV_OK;
}
// ras_save_human_info_to_Pop_info_prev_gen (:3211-3236): called where the reference calls it, behind the migration
int gev_save_prev_gen(gev_ctx* c, int pop, const double* phen_shift)
{
    GEVC(check_idx(c, pop, 0));
    PopState& P = c->pop[pop];
    if (!P.gen0 || !P.comp_ok) return fail(GEV_ESTATE, "save_prev_gen: population %d has no phenotype components of its current individuals (gev_generation_phenotypes)", pop);
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t n = P.n_people;
    if (phen_shift) GEVC(upload_table(c, c->ph.shift, phen_shift, c->nphen, st));
    GEVC(P.d_prev.ensure((size_t)c->nphen * 2 * n, st));
    hipLaunchKernelGGL(k_ph_save_prev, dim3((unsigned)ceil_div(n, 256), (unsigned)c->nphen), dim3(256), 0, st, P.d_comp[P.cbuf], n,
                       phen_shift ? c->ph.shift : (const double*)nullptr, P.d_prev);
    KCHECK();
    P.prev_n = n; P.prev_ok = true;
    return GEV_OK;
}
int gev_upload_prev_gen(gev_ctx* c, int pop, const double* phen, const double* parental_effect, size_t n)
{
    GEVC(check_idx(c, pop, 0));
    if (!n) return fail(GEV_EINVAL, "upload_prev_gen: empty record");
    PopState& P = c->pop[pop];
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPC(hipStreamSynchronize(st));                         // (a phenotype step that reads the old record may be in flight)
    const size_t nphen = (size_t)c->nphen;
    GEVC(P.d_prev.ensure(nphen * 2 * n, st));
    HIPC(hipMemsetAsync(P.d_prev.p, 0, nphen * 2 * n * sizeof(double), st));
    for (size_t p = 0; p < nphen; p++) {
        if (phen) HIPC(hipMemcpyAsync(P.d_prev + (p * 2 + 0) * n, phen + p * n, n * sizeof(double), hipMemcpyHostToDevice, st));
        if (parental_effect) HIPC(hipMemcpyAsync(P.d_prev + (p * 2 + 1) * n, parental_effect + p * n, n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIPC(hipStreamSynchronize(st));
    P.prev_n = n; P.prev_ok = true;
    return GEV_OK;
}
// test hook: the first attempt of every following gev_generation_phenotypes / gev_scale_ad_compute_gef starts with far too few
// candidate pairs (on != 0); *reruns = steps and calls that were enqueued again, over the context's life
int gev_dbg_phenotype_knobs(gev_ctx* c, int short_candidates, unsigned long long* reruns)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    c->ph.short_candidates = short_candidates != 0;
    if (short_candidates) c->ph.cand_shift = 0;
    if (reruns) *reruns = c->ph.reruns;
    return GEV_OK;
}
// ---- pedigree ids on the device (gev_pedigree.h) ---------------------------------------------
int gev_set_track_pedigree(gev_ctx* c, int on)
{
    GEVC(check_not_pending(c));
    if (on != 0 && on != 1) return fail(GEV_EINVAL, "set_track_pedigree: %d is neither 0 nor 1", on);
    for (const PopState& P : c->pop) if (P.gen0) return fail(GEV_ESTATE, "set_track_pedigree: call it before gev_init_gen0");
    c->track_pedigree = on != 0;
    return GEV_OK;
}
static int check_pedigree(gev_ctx* c, int pop, const char* who)
{
    GEVC(check_idx(c, pop, 0));
    if (!c->track_pedigree) return fail(GEV_ESTATE, "%s: the context does not track pedigree ids (gev_set_track_pedigree)", who);
    if (!c->pop[pop].gen0) return fail(GEV_ESTATE, "%s: population %d has no current generation", who, pop);
    return GEV_OK;
}
int gev_download_pedigree(gev_ctx* c, int pop, int64_t* ids)
{
    GEVC(check_pedigree(c, pop, "download_pedigree"));
    if (!ids) return fail(GEV_EINVAL, "download_pedigree: null output");
    PopState& P = c->pop[pop];
    if (!P.ids_ok) return fail(GEV_ESTATE, "download_pedigree: population %d's pedigree ids were dropped when its rows changed (gev_upload_pedigree restores them)", pop);
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t n = P.n_people;
    const u32* logical = nullptr;
    if (!P.logical.empty()) { GEVC(h2d(c, c->d_logical, P.logical.data(), n)); logical = c->d_logical; }
    GEVC(c->d_tmp.ensure(n * PED_FIELDS * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_ped_records, dim3((unsigned)ceil_div(n * PED_FIELDS, 256)), dim3(256), 0, st, P.d_ids[P.ibuf], P.ids_stride[P.ibuf],
                       logical, n, c->d_tmp.as<int64_t>());
    KCHECK();
    HIPC(hipMemcpyAsync(ids, c->d_tmp.p, n * PED_FIELDS * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
int gev_upload_pedigree(gev_ctx* c, int pop, const int64_t* ids)
{
    GEVC(check_pedigree(c, pop, "upload_pedigree"));
    if (!ids) return fail(GEV_EINVAL, "upload_pedigree: null ids");
    PopState& P = c->pop[pop];
    HIPC(hipSetDevice(c->device));
    // planes by physical row (rows no position names any more keep -1)
    const size_t n = P.n_people, rows = P.logical.empty() ? n : P.n_phys;
    std::vector<int64_t> planes(PED_FIELDS * rows, -1);
    for (size_t i = 0; i < n; i++) {
        const size_t r = P.logical.empty() ? i : P.logical[i];
        if (r >= rows) return fail(GEV_EDEVICE, "upload_pedigree: position %zu names row %zu of %zu (internal error)", i, r, rows);
        for (int f = 0; f < PED_FIELDS; f++) planes[f * rows + r] = ids[i * PED_FIELDS + f];
    }
    GEVC(h2d(c, P.d_ids[P.ibuf], planes.data(), planes.size()));
    P.ids_stride[P.ibuf] = rows; P.ids_ok = true;
    return GEV_OK;
}
// ---- Population::ras_save_human_info on the device (gev_fmt_g.h, k_info_rows) ------------------
static int fmt_ready(gev_ctx* c)
{
    if (c->fm.ready) return GEV_OK;
    GEVC(h2d(c, c->fm.tables, &gev_fmt_host_tables(), 1));
    c->fm.ready = true;
    return GEV_OK;
}
int gev_format_info_text(gev_ctx* c, int pop, size_t ind_begin, size_t n_ind, int with_header, char* out, size_t out_bytes, size_t* bytes_written)
{
    GEVC(check_idx(c, pop, 0));
    if (!bytes_written) return fail(GEV_EINVAL, "format_info_text: null bytes_written");
    *bytes_written = 0;
    const u32 nphen = (u32)c->nphen;
    const size_t lds_bytes = 16 + (size_t)INFO_ROWS * info_row_cap(nphen);
    if (lds_bytes > 65536) return fail(GEV_EUNSUPPORTED, "format_info_text: %u phenotypes: a block of rows is staged in 64 KiB, which holds rows of at most 8", nphen);
    GEVC(check_pedigree(c, pop, "format_info_text"));
    PopState& P = c->pop[pop];
    if (!P.ids_ok) return fail(GEV_ESTATE, "format_info_text: population %d's pedigree ids were dropped when its rows changed (gev_upload_pedigree restores them)", pop);
    if (!P.comp_ok || !P.logical.empty())
        return fail(GEV_ESTATE, "format_info_text: population %d has no phenotype components of its current individuals (gev_generation_phenotypes)", pop);
    if (c->ph.pending && c->ph.pop == pop && c->ph.epoch == P.layout_epoch)
        return fail(GEV_ESTATE, "format_info_text: the phenotype step of population %d is outstanding: call gev_phenotypes_result first", pop);
    if (!P.sel_ok) return fail(GEV_ESTATE, "format_info_text: population %d has no selection values of its current generation on the device (gev_compute_selection)", pop);
    const size_t n = P.n_people;
    if (ind_begin > n || n_ind > n - ind_begin) return fail(GEV_EINVAL, "format_info_text: individuals [%zu,%zu) beyond n_people=%zu", ind_begin, ind_begin + n_ind, n);
    std::string hdr;
    if (with_header) {
        hdr = "ID ID_Father ID_Mother ID_Fathers_Father ID_Fathers_Mother ID_Mothers_Father ID_Mothers_Mother sex";
        for (u32 p = 0; p < nphen; p++) for (const char* q = "ADGCEFP"; *q; q++) { hdr += " ph" + std::to_string(p + 1) + "_"; hdr += *q; }
        hdr += " MV SV SV_f\n";
    }
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    u64 total = 0;
    const size_t nb = ceil_div(n_ind, INFO_ROWS);
    gev_ctx::FmtState& F = c->fm;
    const int64_t* ids = P.d_ids[P.ibuf]; const size_t ids_stride = P.ids_stride[P.ibuf];
    const uint8_t* sex = P.d_sex[P.cur];
    const double* comp = P.d_comp[P.cbuf]; const double* sel = P.d_sel[P.sbuf];
    if (n_ind) {
        GEVC(fmt_ready(c));
        GEVC(F.lens.ensure(n_ind, st)); GEVC(F.bsum.ensure(nb, st)); GEVC(F.boff.ensure((nb + 1), st));
        hipLaunchKernelGGL(k_info_rows<false>, dim3((unsigned)nb), dim3(INFO_ROWS), 0, st, F.tables, ids, ids_stride, sex, comp, sel, n, nphen,
                           ind_begin, n_ind, F.lens, F.bsum, (const u64*)nullptr, (char*)nullptr);
        hipLaunchKernelGGL(k_info_scan64, dim3(1), dim3(256), 0, st, F.bsum, nb, F.boff);
        KCHECK();
        HIPC(hipMemcpyAsync(&total, F.boff + nb, sizeof total, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
    }
    const size_t need = hdr.size() + (size_t)total;
    *bytes_written = need;
    if (!out) return GEV_OK;
    if (out_bytes < need) return fail(GEV_EINVAL, "format_info_text: buffer of %zu bytes, %zu needed", out_bytes, need);
    memcpy(out, hdr.data(), hdr.size());
    if (!total) return GEV_OK;
    GEVC(c->d_text.ensure((size_t)total + 16, st));
    hipLaunchKernelGGL(k_info_rows<true>, dim3((unsigned)nb), dim3(INFO_ROWS), lds_bytes, st, F.tables, ids, ids_stride, sex, comp, sel, n, nphen,
                       ind_begin, n_ind, F.lens, (u32*)nullptr, F.boff, c->d_text.as<char>());
    KCHECK();
    HIPC(hipMemcpyAsync(out + hdr.size(), c->d_text.p, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    return GEV_OK;
}
int gev_dbg_format_g(gev_ctx* c, const double* x, size_t n, char* out, unsigned long long* n_exact)
{
    GEVC(check_not_pending(c));
    if (n && (!x || !out)) return fail(GEV_EINVAL, "dbg_format_g: null argument");
    if (n_exact) *n_exact = 0;
    if (!n) return GEV_OK;
    HIPC(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    GEVC(fmt_ready(c));
    gev_ctx::FmtState& F = c->fm;
    GEVC(F.x.ensure(n, st)); GEVC(c->d_text.ensure(n * 16, st)); GEVC(F.cnt.ensure(1, st));
    HIPC(hipMemcpyAsync(F.x.p, x, n * sizeof(double), hipMemcpyHostToDevice, st));
    HIPC(hipMemsetAsync(F.cnt.p, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_dbg_format_g, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, F.tables, F.x, n,
                       c->d_text.as<uint4>(), F.cnt);
    KCHECK();
    unsigned long long cnt = 0;
    HIPC(hipMemcpyAsync(out, c->d_text.p, n * 16, hipMemcpyDeviceToHost, st));
    HIPC(hipMemcpyAsync(&cnt, F.cnt.p, sizeof cnt, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (n_exact) *n_exact = cnt;
    return GEV_OK;
}
// the same header compiled for the host: no device, no context
int gev_dbg_format_g_host(const double* x, size_t n, char* out, unsigned long long* n_exact)
{
    if (n && (!x || !out)) return fail(GEV_EINVAL, "dbg_format_g_host: null argument");
    const GevFmtTables& T = gev_fmt_host_tables();
    unsigned long long cnt = 0;
    for (size_t i = 0; i < n; i++) {
        GevG o; u32 ex = 0;
        gev_fmt_g(&T, x[i], o, &ex);
        memcpy(out + 16 * i, &o.lo, 8); memcpy(out + 16 * i + 8, &o.hi, 8);
        cnt += ex;
    }
    if (n_exact) *n_exact = cnt;
    return GEV_OK;
}
// ---- Simulation::ras_write_hap_to_interval_format on the device (gev_fmt_int.h, k_int_rows) ------------------
int gev_set_founder_names(gev_ctx* c, int root_pop, const char* bytes, const uint32_t* offsets, size_t n_individuals)
{
    if (!c) return fail(GEV_EINVAL, "null context");
    if (root_pop < 0 || root_pop >= c->n_pop) return fail(GEV_EINVAL, "set_founder_names: population index %d out of range", root_pop);
    if (!offsets || (!bytes && offsets[n_individuals] != offsets[0])) return fail(GEV_EINVAL, "set_founder_names: null argument");
    if (n_individuals >= 0xffffffffull) return fail(GEV_EINVAL, "set_founder_names: %zu names", n_individuals);
    for (size_t i = 0; i < n_individuals; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(GEV_EINVAL, "set_founder_names: the offsets decrease at name %zu", i);
        if (offsets[i + 1] - offsets[i] > GEV_INT_NAME_MAX)
            return fail(GEV_EUNSUPPORTED, "set_founder_names: name %zu of population %d has %u bytes: at most %d fit a staged line", i, root_pop, offsets[i + 1] - offsets[i], GEV_INT_NAME_MAX);
    }
    gev_ctx::IntState& I = c->iv;
    if (I.host.size() != (size_t)c->n_pop) I.host.resize(c->n_pop);
    gev_ctx::IntState::Names& N = I.host[root_pop];
    N.offs.resize(n_individuals + 1);
    for (size_t i = 0; i <= n_individuals; i++) N.offs[i] = offsets[i] - offsets[0];
    N.bytes.clear();
    if (bytes) N.bytes.assign((const unsigned char*)bytes + offsets[0], (const unsigned char*)bytes + offsets[n_individuals]);
    N.set = true; I.uploaded = false;
    return GEV_OK;
}
static int int_names_ready(gev_ctx* c)
{
    gev_ctx::IntState& I = c->iv;
    if (I.uploaded) return GEV_OK;
    if (I.d_bytes.size() != (size_t)c->n_pop) { I.d_bytes.resize(c->n_pop); I.d_offs.resize(c->n_pop); }
    std::vector<IntNames> tab(c->n_pop);
    for (int p = 0; p < c->n_pop; p++) {
        const gev_ctx::IntState::Names& N = I.host[p];
        GEVC(h2d(c, I.d_bytes[p], N.bytes.data(), N.bytes.size())); GEVC(h2d(c, I.d_offs[p], N.offs.data(), N.offs.size()));
        tab[p] = IntNames{I.d_bytes[p], I.d_offs[p], (u64)(N.offs.size() - 1)};
    }
    GEVC(h2d(c, I.d_names, tab.data(), tab.size()));
    I.uploaded = true;
    return GEV_OK;
}
int gev_format_interval_text(gev_ctx* c, int pop, int chr, int chr_label, size_t ind_begin, size_t n_ind, int with_header, const int64_t* ids,
                             char* out, size_t out_bytes, size_t* bytes_written)
{
    const char* who = "format_interval_text";
    if (!bytes_written) return fail(GEV_EINVAL, "%s: null bytes_written", who);
    *bytes_written = 0;
    GEVC(output_begin(c, pop, chr, who, false));
    if (!c->track_intervals) return fail(GEV_ESTATE, "%s: interval tracking is disabled (gev_set_track_intervals)", who);
    gev_ctx::IntState& I = c->iv;
    for (int p = 0; p < c->n_pop; p++)
        if ((size_t)p >= I.host.size() || !I.host[p].set) return fail(GEV_ESTATE, "%s: the founder names of root population %d were never set (gev_set_founder_names)", who, p);
    PopState& P = c->pop[pop]; ChrState& cs = P.st[chr];
    if (!ids) {
        if (!c->track_pedigree) return fail(GEV_ESTATE, "%s: ids == NULL and the context does not track pedigree ids (gev_set_track_pedigree)", who);
        if (!P.ids_ok) return fail(GEV_ESTATE, "%s: ids == NULL and population %d's pedigree ids were dropped when its rows changed (gev_upload_pedigree restores them)", who, pop);
    }
    GEVC(ensure_csr(c, pop));
    const size_t n = P.n_people;
    if (ind_begin > n || n_ind > n - ind_begin) return fail(GEV_EINVAL, "%s: individuals [%zu,%zu) beyond n_people=%zu", who, ind_begin, ind_begin + n_ind, n);
    const size_t hdr = with_header ? strlen(GEV_INT_HEADER) : 0;
    hipStream_t st = c->stream;
    const u32* poff = cs.poff[P.cur]; const gev_part* parts = cs.parts[P.cur];
    const size_t row0 = 2 * ind_begin, row1 = 2 * (ind_begin + n_ind);
    u32 pr[2] = {0, 0};
    if (n_ind) {
        HIPC(hipMemcpyAsync(&pr[0], poff + row0, sizeof(u32), hipMemcpyDeviceToHost, st)); HIPC(hipMemcpyAsync(&pr[1], poff + row1, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
    }
    const size_t np = pr[1] - pr[0], nb = ceil_div(np, INT_PARTS);
    u64 total = 0;
    const int64_t* d_ids = nullptr; size_t id_ind0 = 0;
    if (np) {
        GEVC(int_names_ready(c));
        if (ids) { GEVC(h2d(c, I.ids, ids, n_ind)); d_ids = I.ids; id_ind0 = ind_begin; }
        else d_ids = P.d_ids[P.ibuf] + PED_ID * P.ids_stride[P.ibuf];
        GEVC(I.lens.ensure(np, st)); GEVC(I.bsum.ensure(nb, st)); GEVC(I.boff.ensure((nb + 1), st)); GEVC(I.flag.ensure(1, st));
        HIPC(hipMemsetAsync(I.flag.p, 0, sizeof(u32), st));
        hipLaunchKernelGGL(k_int_rows<false>, dim3((unsigned)nb), dim3(INT_PARTS), INT_SCAN_BYTES, st, poff, parts, row0, row1, pr[0], pr[1], d_ids, id_ind0, chr_label,
                           I.d_names, c->n_pop, 0u, I.lens, I.bsum, (const u64*)nullptr, (u64)0, (char*)nullptr, I.flag);
        hipLaunchKernelGGL(k_info_scan64, dim3(1), dim3(256), 0, st, I.bsum, nb, I.boff);
        KCHECK();
        u32 flag = 0;
        HIPC(hipMemcpyAsync(&total, I.boff + nb, sizeof total, hipMemcpyDeviceToHost, st));
        HIPC(hipMemcpyAsync(&flag, I.flag.p, sizeof flag, hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        if (flag) return fail(GEV_EINVAL, "%s: a part of population %d names a founder (hap_index / 2) beyond the names of its root population", who, pop);
    }
    const size_t need = hdr + (size_t)total;
    *bytes_written = need;
    if (!out) return GEV_OK;
    if (out_bytes < need) return fail(GEV_EINVAL, "%s: buffer of %zu bytes, %zu needed", who, out_bytes, need);
    memcpy(out, GEV_INT_HEADER, hdr);
    if (!total) return GEV_OK;
    // the text leaves in runs of blocks whose largest possible lines stay within 256 MB of staging
    const size_t chunk = output_chunk(c, 256u << 20, (size_t)INT_PARTS * GEV_INT_LINE_MAX);
    std::vector<u64> boff;
    if (nb > chunk) {
        boff.resize(nb + 1);
        HIPC(hipMemcpyAsync(boff.data(), I.boff.p, (nb + 1) * sizeof(u64), hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
    }
    for (size_t b0 = 0; b0 < nb; b0 += chunk) {
        const size_t b1 = std::min(nb, b0 + chunk);
        const u64 o0 = boff.empty() ? 0 : boff[b0], o1 = boff.empty() ? total : boff[b1];
        if (o1 == o0) continue;
        GEVC(copy_out_text(c, (size_t)(o1 - o0), out + hdr + o0, [&] {
            hipLaunchKernelGGL(k_int_rows<true>, dim3((unsigned)(b1 - b0)), dim3(INT_PARTS), INT_SCAN_BYTES + INT_LDS_BYTES, st, poff, parts, row0, row1, pr[0], pr[1], d_ids, id_ind0, chr_label,
                               I.d_names, c->n_pop, (u32)b0, I.lens, (u32*)nullptr, I.boff, o0, c->d_text.as<char>(),
                               (u32*)nullptr);
        }));
    }
    return GEV_OK;
}
// the same header compiled for the host: no device, no context
int gev_dbg_format_interval_text_host(const gev_part* parts, const uint64_t* hap_offsets, size_t n_ind, const int64_t* ids, int chr_label,
                                      const char* const* name_bytes, const uint32_t* const* name_offsets, const size_t* n_names, int n_root_pop,
                                      int with_header, char* out, size_t out_bytes, size_t* bytes_written)
{
    const char* who = "dbg_format_interval_text_host";
    if (!bytes_written) return fail(GEV_EINVAL, "%s: null bytes_written", who);
    *bytes_written = 0;
    if (n_ind && (!hap_offsets || !ids)) return fail(GEV_EINVAL, "%s: null argument", who);
    const size_t hdr = with_header ? strlen(GEV_INT_HEADER) : 0;
    for (int pass = 0; pass < 2; pass++) {
        size_t at = hdr;
        for (size_t r = 0; r < 2 * n_ind; r++)
            for (u64 q = hap_offsets[r]; q < hap_offsets[r + 1]; q++) {
                if (!parts) return fail(GEV_EINVAL, "%s: null parts", who);
                const gev_part& p = parts[q];
                const int rp = p.root_population;
                if (rp < 0 || rp >= n_root_pop || !name_offsets || !name_offsets[rp] || !n_names) return fail(GEV_EINVAL, "%s: root population %d has no names", who, rp);
                const u64 k = p.hap_index >> 1;
                if (k >= n_names[rp]) return fail(GEV_EINVAL, "%s: a part names founder %llu beyond the %zu names of root population %d", who, (unsigned long long)k, n_names[rp], rp);
                const u32 o0 = name_offsets[rp][k], nlen = name_offsets[rp][k + 1] - o0;
                if (nlen > GEV_INT_NAME_MAX) return fail(GEV_EUNSUPPORTED, "%s: a name of %u bytes", who, nlen);
                const GevIntLine l{(u64)(ids[r >> 1] + 1), p.st, p.en, p.hap_index + 1, (u32)(rp + 1), (u32)(r & 1u), chr_label};
                if (pass) { GevIntMemSink s{out + at}; gev_int_line(s, 0, l, (const unsigned char*)name_bytes[rp] + o0, nlen); }
                at += gev_int_line_len(l, nlen);
            }
        if (!pass) {
            *bytes_written = at;
            if (!out) return GEV_OK;
            if (out_bytes < at) return fail(GEV_EINVAL, "%s: buffer of %zu bytes, %zu needed", who, out_bytes, at);
            memcpy(out, GEV_INT_HEADER, hdr);
        }
    }
    return GEV_OK;
}
int gev_set_track_intervals(gev_ctx* c, int on)
{
    if (!c) return fail(GEV_EINVAL, "null");
    if (c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first");
    if (c->track_intervals == (on != 0)) return GEV_OK;
    for (int p = 0; p < c->n_pop; p++) if (c->pop[p].gen0) { GEVC(ensure_csr(c, p)); lists_changed_in_csr(c, c->pop[p]); }   // the pieces are rebuilt with / without the interval tables
    c->track_intervals = on != 0;
    return GEV_OK;
}
int gev_list_stats(gev_ctx* c, int pop, int chr, unsigned long long out[10])
{
    GEVC(check_idx(c, pop, chr));
    if (!out) return fail(GEV_EINVAL, "list_stats: null argument");
    const ChrState::LpState& lp = c->pop[pop].st[chr].lp;
    out[0] = lp.imports; out[1] = lp.p_used; out[2] = lp.m_used; out[3] = lp.parena.capacity(); out[4] = lp.marena.capacity();
    out[5] = lp.nseg; out[6] = lp.p_last; out[7] = lp.m_last; out[8] = lp.compactions; out[9] = 0;
    return GEV_OK;
}
int gev_redo_count(gev_ctx* c, unsigned long long* n) { if (!c || !n) return fail(GEV_EINVAL, "null"); *n = c->redo_count; return GEV_OK; }
int gev_dbg_pool_stats(gev_ctx* c, int pop, unsigned long long out[2])
{
    if (!c || !out) return fail(GEV_EINVAL, "null");
    GEVC(check_idx(c, pop, 0));
    out[0] = 0; out[1] = c->redo_pool_count;
    for (int k = 0; k < c->nchr; k++) if (c->chr_active[k]) out[0] = std::max(out[0], c->pop[pop].st[k].pool_rebuilds);
    return GEV_OK;
}
int gev_set_overlap(gev_ctx* c, int on)
{
    if (!c) return fail(GEV_EINVAL, "null");
    if (on != 0 && on != 1) return fail(GEV_EINVAL, "set_overlap: %d is neither 0 (serialised) nor 1 (overlap)", on);
    GEVC(gev_sync(c));
    c->serialize = on == 0;
    return GEV_OK;
}
int gev_set_cv_stitch_form(gev_ctx* c, int form) { if (c && c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first"); if (!c || form < 0 || form > 2) return fail(GEV_EINVAL, "CV stitch form must be 0 (automatic), 1 (a half-wave per row) or 2 (eight lanes per row where the planes allow it)"); c->cv_stitch_form = form; return GEV_OK; }
int gev_dbg_cv_stitch_launches(gev_ctx* c, unsigned long long launches[2]) { if (!c || !launches) return fail(GEV_EINVAL, "null argument"); launches[0] = c->cv_stitch_launches[0]; launches[1] = c->cv_stitch_launches[1]; return GEV_OK; }
int gev_set_stitch_mode(gev_ctx* c, int mode) { if (c && c->pend.active) return fail(GEV_ESTATE, "a gev_reproduce_begin is pending: call gev_reproduce_end first"); if (!c || mode < 0 || mode > 1) return fail(GEV_EINVAL, "stitch mode must be 0 (work list of the segments to write) or 1 (gamete-major)"); c->stitch_mode = mode; return GEV_OK; }

// ---- diagnostics (tests only; no simulation state involved) --------------------------------
__global__ void __launch_bounds__(64) k_dbg_rand(const GevRngTables* __restrict__ T, u32 seed, u32 n, int* __restrict__ out)
{
    GlibcWave g; g.seed(T, seed);
    for (u32 i = 0; i < n; i++) { const u32 v = g.out(T, i); if (threadIdx.x == 0) out[i] = (int)v; }
}
// one gamete of ras_sim_loc_rec: breakpoints + the next two rand() outputs
__global__ void __launch_bounds__(64) k_dbg_sim_loc_rec(const GevRngTables* __restrict__ T, const ChrDev* __restrict__ chrs, int chr, u32 seed,
                                                        u64* __restrict__ locs, u32 cap, u32* __restrict__ n_out, int* __restrict__ next2)
{
    const ChrDev& C = chrs[chr];
    GlibcWave g; g.seed(T, seed);
    u32 h = 0;
    wave_scan_hits(T, seed + 1u, C.rthr, C.r_amax, 0, C.R, [&](u32 row) {
        const u64 v = C.rbp[row] + (u64)g.out(T, h) % C.bp_dist;
        if (threadIdx.x == 0 && h < cap) locs[h] = v;
        h++;
    });
    const u32 a = g.out(T, h), b = g.out(T, h + 1);
    if (threadIdx.x == 0) { *n_out = h; next2[0] = (int)a; next2[1] = (int)b; }
}
// every word of the resident plane (dense stitch) against the interval state (k_parts) + the synthetic founder panel
int gev_dbg_verify_planes(gev_ctx* c, int pop, int chr, const uint64_t* founder_seeds, unsigned long long* n_bad_words, unsigned long long* n_bad_parts)
{
    if (c) GEVC(check_dense(c, "dbg_verify_planes"));
    GEVC(check_idx(c, pop, chr));
    GEVC(check_active(c, chr, "dbg_verify_planes"));
    PopState& P = c->pop[pop]; ChrStatic& S = P.cs[chr]; ChrState& cs = P.st[chr];
    if (!P.gen0) return fail(GEV_ESTATE, "dbg_verify_planes: population %d has no current generation", pop);
    if (!c->track_intervals) return fail(GEV_ESTATE, "dbg_verify_planes: interval tracking is disabled");
    if (!founder_seeds || !n_bad_words || !n_bad_parts) return fail(GEV_EINVAL, "dbg_verify_planes: null argument");
    HIPC(hipSetDevice(c->device));
    GEVC(materialize_order(c, pop));
    GEVC(ensure_csr(c, pop));
    GEVC(gev_sync(c));
    hipStream_t st = c->stream;
    const size_t rows = 2 * P.n_people, words = ceil_div(S.L, 32);
    if (!rows || !words) { *n_bad_words = 0; *n_bad_parts = 0; return GEV_OK; }
    if (ceil_div(rows * words, 256) > 0x7fffffffull) return fail(GEV_EINVAL, "dbg_verify_planes: grid too large");
    // per ROOT population: allele-frequency thresholds of its synthetic panel, its seed, its number of founder haplotypes
    // (a population this context never generated founders for is taken to have as many as this one: same panel shape on every GPU)
    const int np = c->n_pop;
    GEVC(c->d_thr32.ensure((size_t)np * S.L, st));
    std::vector<u64> meta(2 * (size_t)np);
    for (int r = 0; r < np; r++) {
        meta[r] = founder_seeds[r];
        meta[np + r] = c->pop[r].cs[chr].founder_rows ? c->pop[r].cs[chr].founder_rows : S.founder_rows;
        hipLaunchKernelGGL(k_synth_thresholds, dim3((unsigned)ceil_div(S.L, 256)), dim3(256), 0, st, c->d_thr32 + (size_t)r * S.L, S.L, founder_seeds[r]);
    }
    GEVC(h2d(c, c->d_map, meta.data(), meta.size() * sizeof(u64)));
    GEVC(c->d_flag.ensure(16, st));
    HIPC(hipMemsetAsync(c->d_flag.p, 0, 16, st));
    hipLaunchKernelGGL(k_verify_plane, dim3((unsigned)ceil_div(rows * words, 256)), dim3(256), 0, st, cs.poff[P.cur], cs.parts[P.cur], rows,
                       S.d_pos, (u32)S.L, row_map(P, chr), c->d_thr32, c->d_map.as<u64>(), np, c->d_map.as<u64>() + np,
                       c->d_flag.as<unsigned long long>());
    KCHECK();
    unsigned long long h[2] = {0, 0};
    HIPC(hipMemcpyAsync(h, c->d_flag.p, 16, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    *n_bad_words = h[0]; *n_bad_parts = h[1];
    return GEV_OK;
}
// Exhaustive check of the FP64 prefilter of the batched sampling kernels (gev_sample8.h:scan_candidates) over engine states
// [x_begin, x_end) and all SB_M multipliers of a block (smp_scan_multiplier, the same definition the kernel's tables are built
// from): with the exact high digit x2 = x * c_m mod M and F = floor(x2 * 2^16 / M), the SB_PF_BITS = 16 low mantissa bits L of
// fma(x, fl(c_m / M), SB_PF_BIAS) must satisfy d = L - SB_PF_OFF - F in [-SB_PF_DNEG, SB_PF_DPOS] = {0, 1} (mod 2^16): then every
// draw whose x2 is <= amax passes L < floor(amax * 2^16 / M) + SB_PF_MARGIN, for every amax, and no L wraps below 0.  The scan
// takes its offset and margin from the same constants, so a violation of the band is a violation of the kernel's test.
// out[0] = violations, out[1] = largest d, out[2] = largest -d.
__global__ void __launch_bounds__(256) k_dbg_prefilter_sweep(const GevRngTables* __restrict__ Tg, u32 x_begin, u32 x_end, unsigned long long* __restrict__ out)
{
    __shared__ double s_kd[SB_M]; __shared__ u32 s_ci[SB_M];
    for (u32 i = threadIdx.x; i < SB_M; i += blockDim.x) smp_scan_multiplier(Tg, i, s_ci[i], s_kd[i]);
    __syncthreads();
    const double C = SB_PF_BIAS;
    unsigned long long bad = 0; int dpos = 0, dneg = 0;
    for (u64 x = (u64)x_begin + (u64)blockIdx.x * 256 + threadIdx.x; x < x_end; x += (u64)gridDim.x * 256) {
        const double xd = (double)(u32)x;
        for (u32 j = 0; j < SB_M; j++) {
            const u32 x2 = mulmod31((u32)x, s_ci[j]);
            const u32 F = (u32)(((u64)x2 << SB_PF_BITS) / 2147483647ull);
            const u32 L = (u32)__double2loint(__fma_rn(xd, s_kd[j], C)) & SB_PF_MASK;
            int d = (int)((L - (u32)SB_PF_OFF - F) & SB_PF_MASK);
            if (d >= (1 << (SB_PF_BITS - 1))) d -= (1 << SB_PF_BITS);
            if (d < -SB_PF_DNEG || d > SB_PF_DPOS) bad++;
            dpos = max(dpos, d); dneg = max(dneg, -d);
        }
    }
    if (bad) atomicAdd(&out[0], bad);
    atomicMax(&out[1], (unsigned long long)dpos); atomicMax(&out[2], (unsigned long long)dneg);
}
int gev_dbg_prefilter_sweep(gev_ctx* c, uint32_t x_begin, uint32_t x_end, unsigned long long out[3])
{
    if (!c || !out) return fail(GEV_EINVAL, "null");
    if (x_begin < 1 || x_end > 2147483647u || x_begin > x_end) return fail(GEV_EINVAL, "dbg_prefilter_sweep: engine states are 1 .. 2^31-2");
    HIPC(hipSetDevice(c->device));
    GEVC(c->d_flag.ensure(32, c->stream));
    HIPC(hipMemsetAsync(c->d_flag.p, 0, 24, c->stream));
    hipLaunchKernelGGL(k_dbg_prefilter_sweep, dim3(8192), dim3(256), 0, c->stream, c->d_tables, x_begin, x_end, c->d_flag.as<unsigned long long>());
    KCHECK();
    HIPC(hipMemcpyAsync(out, c->d_flag.p, 24, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return GEV_OK;
}
int gev_dbg_tables(void* out, size_t bytes)
{
    if (bytes != sizeof(GevRngTables)) return fail(GEV_EINVAL, "gev_dbg_tables: expected %zu bytes", sizeof(GevRngTables));
    GevRngTables T; gev_build_rng_tables(T); memcpy(out, &T, sizeof T); return GEV_OK;
}
int gev_dbg_threshold(double p, uint32_t out[4])
{
    GevThr t;
    if (!gev_make_threshold(p, t)) return fail(GEV_EUNSUPPORTED, "window wider than 2");
    out[0] = t.a_lo; out[1] = t.a_hi; out[2] = t.b0; out[3] = t.b1; return GEV_OK;
}
double gev_dbg_canonical(uint32_t a, uint32_t b) { return gev_canonical(a, b); }
int gev_dbg_rand(gev_ctx* c, uint32_t seed, uint32_t n, int* out)
{
    if (!c || !out) return fail(GEV_EINVAL, "null");
    HIPC(hipSetDevice(c->device));
    GEVC(c->d_tmp.ensure(std::max<size_t>(n, 4) * sizeof(int), c->stream));
    hipLaunchKernelGGL(k_dbg_rand, dim3(1), dim3(64), 0, c->stream, c->d_tables, seed, n, c->d_tmp.as<int>());
    KCHECK();
    HIPC(hipMemcpyAsync(out, c->d_tmp.p, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return GEV_OK;
}
int gev_dbg_ad_path(gev_ctx* c, int* path)
{
    if (!c || !path) return fail(GEV_EINVAL, "null");
    *path = c->ad_path;
    return GEV_OK;
}
int gev_dbg_sampling_path(gev_ctx* c, int* path)
{
    if (!c || !path) return fail(GEV_EINVAL, "null");
    *path = c->sampling_path;
    return GEV_OK;
}
int gev_dbg_sim_loc_rec(gev_ctx* c, int pop, int chr, uint32_t seed, uint64_t* locs, uint32_t cap, uint32_t* n, int next2[2])
{
    GEVC(check_idx(c, pop, chr));
    HIPC(hipSetDevice(c->device));
    GEVC(finalize_static(c, pop));
    GEVC(c->d_tmp.ensure((size_t)cap * 8 + 64, c->stream));
    u64* dl = c->d_tmp.as<u64>(); u32* dn = (u32*)(dl + cap); int* dx = (int*)(dn + 2);
    hipLaunchKernelGGL(k_dbg_sim_loc_rec, dim3(1), dim3(64), 0, c->stream, c->d_tables, c->pop[pop].d_chrdev, chr, seed, dl, cap, dn, dx);
    KCHECK();
    HIPC(hipMemcpyAsync(n, dn, 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(next2, dx, 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipMemcpyAsync(locs, dl, (size_t)std::min(*n, cap) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return GEV_OK;
}

} // extern "C"
