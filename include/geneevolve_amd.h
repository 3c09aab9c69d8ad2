/* geneevolve_amd.h -- C-ABI of the MI355X-native GeneEvolve reproduction hot path.
 *
 * The reference (MMesbahU/GeneEvolve) has no plugin/FFI interface; the seam is the set of
 * private members of class Simulation (reference src/Simulation.h:64-144) listed below.  A
 * maintainer replaces their bodies with calls to this library (INTEGRATION.md shows the
 * patch).  Every entry point names the reference code it replaces.
 *
 *   reference seam (src/Simulation.h)                      entry point here
 *   ------------------------------------------------------ ---------------------------------
 *   ras_init_parameters (readers, src/Simulation.cpp:164)  gev_set_rmap / gev_set_mutmap /
 *                                                          gev_set_snps / gev_set_cvs /
 *                                                          gev_upload_founders / gev_upload_cv_founders
 *   bool ras_initial_human_gen0(int ipop)          :86     gev_init_gen0
 *   bool random_mate(int ipop,int gen_ind)         :78     gev_random_mate
 *   unsigned ras_glob_seed(void)                   :67     gev_glob_seeds; inside gev_generation_begin
 *   sim_next_generation: random_mate -> reproduce -> ras_compute_AD as one unit     gev_generation_begin / _end
 *   std::vector<Human> reproduce(int,int)          :81     gev_reproduce
 *   bool ras_compute_AD(int ipop,int gen_num)      :80     gev_compute_ad
 *   bool ras_do_migration(int gen_ind)             :71     gev_migrate (+ gev_export_rows /
 *                                                          gev_import_rows across GPUs)
 *   ras_convert_interval_to_hap_matrix             :105    gev_download_haps
 *   ras_write_hap_to_interval_format               :116    gev_download_intervals
 *
 * Conventions (mirroring the reference's): every call returns 0 on success and a negative
 * GEV_E* code on failure (the reference returns bool false and prints one line; the line is
 * available from gev_last_error()).  No exceptions cross the boundary.  The caller owns every
 * host buffer it passes; the library owns all device memory.  Exactly one host thread drives
 * one context (the reference is single threaded).  One context lives on one GPU; one process
 * per GPU.
 *
 * Bit packing of every genotype buffer crossing the boundary: haplotype-major rows
 * (row = 2*individual + chromatid, as Hap_SNP.hap in reference src/format_hap.h:18-31),
 * locus ii of a row is bit (ii & 63) of 64-bit little-endian word ii >> 6; rows are
 * `row_stride_words` words apart; pad bits are zero.
 *
 * RNG coupling: the host keeps drawing Simulation::ras_glob_seed()
 * (src/Simulation.cpp:17-21) exactly as the reference does and hands the values in:
 * 1 value per gev_init_gen0, 1 per gev_reproduce plus 1 per (offspring, chromosome) when a
 * mutation map is loaded (the draw inside ras_add_mutation, src/Simulation.cpp:2500).
 */
#ifndef GENEEVOLVE_AMD_H
#define GENEEVOLVE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEV_OK          0
#define GEV_EINVAL     -1   /* bad argument / inconsistent sizes                                   */
#define GEV_ESTATE     -2   /* call order violated (e.g. reproduce before init_gen0)               */
#define GEV_EDEVICE    -3   /* HIP runtime error, no device, out of device memory                  */
#define GEV_ENAN       -4   /* "A or D is nan" (reference src/Simulation.cpp:2716-2720)            */
#define GEV_EUNSUPPORTED -5 /* input outside the dense-equivalence preconditions   */
#define GEV_ENOMATE    -6   /* "Error: No one can marry" (reference src/Simulation.cpp:2125-2129)  */

typedef struct gev_ctx gev_ctx;

/* class Couples_Info, reference src/Population.h:165-180.  pos_* index the CURRENT
 * generation of the population by position (not by ID). */
typedef struct gev_couple {
    uint64_t pos_male;
    uint64_t pos_female;
    int32_t  inbreed;        /* != 0: couple is skipped (src/Simulation.cpp:2440) */
    int32_t  num_offspring;
} gev_couple;

/* class part, reference src/Population.h:20-51, without gen0_indv (a pure function of
 * hap_index and root_population: founder id + ".1"/".2", src/Simulation.cpp:3031-3033)
 * and without mutation_pos (see gev_download_mutations). */
typedef struct gev_part {
    uint64_t st;
    uint64_t en;
    uint64_t hap_index;
    int32_t  root_population;
    int32_t  reserved;
} gev_part;

/* one migrant: individual at position src_pos of population src_pop (positions BEFORE the
 * migration step) moves to dst_pop.  Order = the order in which the reference appends
 * migrants (src/Simulation.cpp:971-981). */
typedef struct gev_move {
    int32_t  src_pop;
    int32_t  dst_pop;
    uint64_t src_pos;
} gev_move;

const char* gev_last_error(void);
const char* gev_version(void);

/* device < 0: use the current HIP device.
 * The environment knobs the library reads, all of them (none changes a result).  Tests set them to force rare paths or to compare
 * two forms of a computation; GEV_TRACE_HOST is diagnostic output.  PER CONTEXT, read here and kept in the context (a test may set
 * one, create a context, and set another for the next context of the same process): GEV_OVERLAP, GEV_SAMPLE_BATCHED,
 * GEV_STITCH_MODE, GEV_ALIAS_ROWS, GEV_SEG_CHUNKS, GEV_OVF_CAP, GEV_LIST_HEADROOM, GEV_TABLE_RING_BYTES, GEV_CHAIN_WG, GEV_AD_SHARED,
 * GEV_AD_RP_FAST.  PER CALL, read whenever they are used: GEV_LIST_SEGS, GEV_LIST_ARENA, GEV_CHAIN_MAX_TASKS, GEV_LP_LITERAL,
 * GEV_LP_LANES.  PER PROCESS, read once when the library is loaded: GEV_TRACE_HOST.
 *   GEV_OVERLAP=0|1             initial stream overlap mode (gev_set_overlap; default 1)
 *   GEV_SAMPLE_BATCHED=0        one sampling task per wave (the round-1 kernels) instead of eight in one kernel
 *   GEV_STITCH_MODE=0|1         dense stitch kernel (gev_set_stitch_mode; default 0, the segment work list)
 *   GEV_ALIAS_ROWS=0            write every segment of every gamete row (default 1: a segment without a crossover boundary shares the parental unit)
 *   GEV_SEG_CHUNKS=2^k          16-byte chunks per row segment (default 128 = 2 KiB; a row has at most 64 segments, longer rows get larger ones)
 *   GEV_OVF_CAP=n               initial size of the breakpoint / new-mutation overflow regions (tiny values force the grow-and-enqueue-again path)
 *   GEV_LIST_SEGS=n             most position ranges per row of the shared list pieces (default 32; 1 = one piece per list) -- csrc/gev_lists.h
 *   GEV_LIST_ARENA=n            entries per row of the list-piece arenas (default: a tenth of the device memory, at most 4096 per row)
 *   GEV_LIST_HEADROOM=n         spare list entries per row when a list buffer is sized (default 48; 0: exact, every generation overflows and is enqueued again)
 *   GEV_TABLE_RING_BYTES=n      minimum size of the pinned ring the per-generation work tables are staged through (default 256 KiB)
 *   GEV_CHAIN_WG=0              serial-chain mode (no mutation map) with one wave per link instead of a workgroup
 *   GEV_CHAIN_MAX_TASKS=n       most (offspring, chromosome) tasks accepted without a mutation map (default 4 000 000)
 *   GEV_AD_SHARED=0             several root populations with bit-identical CV effects: per-haplotype a/d lookup anyway (default: the one-population term table)
 *   GEV_AD_RP_FAST=0            several root populations with their own CV effects: per-haplotype a/d lookup in global memory (k_ad_accumulate) even
 *                               when the CV files are in position order (default then: k_ad_accumulate_rp, the piece's values in LDS)
 *   GEV_LP_LITERAL=1            list pieces built by recombine's statements one by one instead of their closed form (cross-check)
 *   GEV_LP_LANES=1|8            new list pieces planned per thread and copied per workgroup (1, the default) or built by eight lanes each (8)
 *   GEV_TRACE_HOST=1            stderr: host time per phase of a generation, the main stream's time by phase, allocations, deferred frees */
int  gev_create(gev_ctx** out, int device, int n_pop, int nchr, int nphen);
void gev_destroy(gev_ctx* ctx);

/* ---- static inputs (what ras_init_parameters loads) -------------------------------------- */
/* rMap + _recom_prob of one chromosome (src/Population.h:183-189, src/Population.cpp:471-480).
 * bp_dist = rMap::bp_dist_in_rmap (src/Population.cpp:396-397). */
int gev_set_rmap(gev_ctx*, int pop, int chr, const uint64_t* bp, const double* recom_prob,
                 size_t R, uint64_t bp_dist);
/* MutationMap of one chromosome (src/Population.h:192-197); rates already range-checked by the
 * reader (src/Population.cpp:458).  M may be 0. */
int gev_set_mutmap(gev_ctx*, int pop, int chr, const uint64_t* bp, const double* rate, size_t M);
/* Legend.pos of the founder panel (src/format_hap.h); must be non-decreasing. */
int gev_set_snps(gev_ctx*, int pop, int chr, const uint64_t* pos, size_t L);
/* CV_INFO of one phenotype x chromosome (src/Population.h:201-208): bp, genetic_value_a,
 * genetic_value_d in FILE order (the A/D sum runs in this order); vd = Phenotype_scheme::_vd.
 * Allowed between generations (not between gev_reproduce_begin / gev_generation_begin and their _end): the next A/D of every
 * population uses the new a, d and vd, including the mean of two root populations' effects for admixed haplotypes.  Once the
 * population has a generation (gev_init_gen0) its CV positions are fixed: other positions (or another count) return
 * GEV_EUNSUPPORTED and change nothing. */
int gev_set_cvs(gev_ctx*, int pop, int phen, int chr, const uint64_t* bp, const double* a,
                const double* d, size_t C, double vd);
/* Hap_SNP.hap founder panel, haplotype-major bit rows (nhap rows x L loci). */
int gev_upload_founders(gev_ctx*, int pop, int chr, const uint64_t* bits, size_t row_stride_words,
                        size_t nhap, size_t L);
/* CV.val of one phenotype x chromosome (src/Population.h:212-216), columns in FILE order. */
int gev_upload_cv_founders(gev_ctx*, int pop, int phen, int chr, const uint64_t* bits,
                           size_t row_stride_words, size_t nhap, size_t C);
/* Synthetic founder panel generated on the device (bench / large parity cases): allele of
 * (hap, locus) ~ Bernoulli(f_locus), f_locus ~ U(0.05,0.5), counter-based hash of `seed`.
 * Not a reference function: SURVEY.md section 8(d) prescribes device-side generation. */
int gev_synth_founders(gev_ctx*, int pop, int chr, size_t nhap, uint64_t seed);
int gev_synth_cv_founders(gev_ctx*, int pop, int phen, int chr, size_t nhap, uint64_t seed);

/* ---- Simulation::ras_initial_human_gen0 (src/Simulation.cpp:3000-3072) --------------------
 * individual i = founder haplotypes 2i, 2i+1 as two whole-chromosome parts
 * [rmap.bp[0], rmap.bp[last]); sex[i] = rand()%2+1 after srand(seed_gen0).
 * sex_out: n_people bytes (1 = male, 2 = female) or NULL. */
int gev_init_gen0(gev_ctx*, int pop, size_t n_people, uint32_t seed_gen0, uint8_t* sex_out);

/* ---- Simulation::reproduce (src/Simulation.cpp:2394-2493) ---------------------------------
 * Replaces the population's current generation by its offspring.
 *  seed_reproduce : the ras_glob_seed() value drawn at :2398
 *  mut_seeds      : NULL when no mutation map is loaded (_mutation_map.size()==0, :2459);
 *                   else the n_people*nchr ras_glob_seed() values drawn inside
 *                   ras_add_mutation (:2500), in call order (offspring-major, chromosome-minor)
 *  n_people       : sum of num_offspring over couples with inbreed==0 (checked)
 *  sex_out        : n_people bytes, Human::sex of each offspring (:2472), or NULL
 * common_sibling (:2481-2484) is host bookkeeping and stays with the host; so do the pedigree ids (:2473-2479) unless the context
 * tracks them (gev_set_track_pedigree).
 *  couples == NULL : the couples the preceding gev_random_mate of `pop` left on the device (n_couples is ignored, n_people must be
 *                   that call's pop_size), or those of the preceding gev_assort_mate (n_people must be its n_offspring).  Returns GEV_ESTATE when the population changed in between (gev_migrate,
 *                   gev_remove_rows, gev_import_rows, or a call that materialised a pending row order): the couples' positions
 *                   would name other rows.
 * Cost note: with a mutation map every (offspring, chromosome) task restarts its rand() chain at srand(mut_seed), so all tasks are
 * sampled in parallel.  WITHOUT one (mut_seeds == NULL) the reference's chain runs through every gamete in order (the seed of a
 * gamete is the rand() output that follows the previous gamete's breakpoints): one wave walks it, about 10 us per gamete, i.e.
 * seconds per generation beyond ~10^5 gametes -- a parity mode for Example1-sized inputs, not a production path. */
int gev_reproduce(gev_ctx*, int pop, const gev_couple* couples, size_t n_couples,
                  uint32_t seed_reproduce, const uint32_t* mut_seeds, size_t n_mut_seeds,
                  size_t n_people, uint8_t* sex_out);

/* Optional head start for the next gev_reproduce of `pop`: crossover / mutation sampling and the rand() seed chain depend
 * on the ras_glob_seed() values and the offspring count only, not on the couples, so they can be enqueued as soon as those
 * are known (random mating with one child per couple: n_people = pop_size) while the host is still forming couples.
 * Returns without waiting.  gev_reproduce called next with the same seed_reproduce, mut_seeds and n_people uses the
 * results; with anything else it samples again.  Same argument checks / errors as gev_reproduce. */
int gev_presample(gev_ctx*, int pop, uint32_t seed_reproduce, const uint32_t* mut_seeds, size_t n_mut_seeds, size_t n_people);
/* gev_reproduce in two halves.  _begin checks and stages the inputs and enqueues the generation's device work; _end waits for it
 * (repeating it with larger buffers if a list capacity was exceeded), publishes the new generation and returns the sexes.
 * gev_reproduce = _begin + _end.  Between the two the host is free -- bench.py forms the next generation's couples there -- but no
 * other call on the context is allowed (GEV_ESTATE). */
int gev_reproduce_begin(gev_ctx*, int pop, const gev_couple* couples, size_t n_couples, uint32_t seed_reproduce,
                        const uint32_t* mut_seeds, size_t n_mut_seeds, size_t n_people);
int gev_reproduce_end(gev_ctx*, uint8_t* sex_out);
/* The sexes of the generation whose sampling gev_presample has enqueued: they come out of the rand() chain of the sampling
 * (src/Simulation.cpp:2472) and depend on nothing else, so a host that mates at random (Simulation::random_mate reads nothing but
 * the sexes) can form the couples of the generation AFTER the one it is about to hand over.  Waits for the sampling kernels only;
 * call it after gev_presample and before the gev_reproduce(_begin) of that generation. */
int gev_presample_sex(gev_ctx*, int pop, uint8_t* sex_out, size_t n_people);

/* ---- Simulation::random_mate (src/Simulation.cpp:2090-2157)  [SURVEY 8(f) row 2] ----------------
 * Forms pop_size couples of the population's current generation on the device, bit for bit as the reference does:
 *  seed                 : the ras_glob_seed() value drawn at :2092
 *  selection_value_func : Human::selection_value_func of every individual [n_people] (:2113), or NULL when every value is 1
 *                         (selection function "none" / generation 0): r < 1 always holds, so the draws of generator(seed)
 *                         cannot change the outcome and are skipped
 *  couples_out          : pop_size Couples_Info records (pos_male, pos_female, inbreed = 0, num_offspring = 1), or NULL
 *  num_*_mate           : the two counts the reference prints (:2122-2123), or NULL
 * Marriageable males / females are compacted in position order (:2109-2118), father and mother of couple i are
 * pos_male[i_f], pos_female[i_m] with i_f / i_m the i-th values of uniform_int_distribution<unsigned long>(0, count-1) on
 * default_random_engine(seed+1) / (seed+2) (:2132-2147).  The sexes are the ones the library itself produced (gev_init_gen0,
 * gev_reproduce; they follow the individuals through gev_migrate / gev_export_rows / gev_import_rows).
 * The couples also stay on the device: the next gev_reproduce of `pop` takes them when its `couples` is NULL, as long as the
 * population's rows are not changed in between.
 * Returns GEV_ENOMATE with the reference's message when no male or no female may marry (:2125-2129). */
int gev_random_mate(gev_ctx*, int pop, uint32_t seed, const double* selection_value_func, size_t pop_size,
                    gev_couple* couples_out, size_t* num_males_mate, size_t* num_females_mate);
/* ---- Simulation::ras_glob_seed (src/Simulation.cpp:17-21) called n times, evaluated on the device ----
 * *engine_state: the state of glob_generator (std::minstd_rand0: `os << glob_generator` prints it, `is >> glob_generator` sets
 * it) before the n calls; on return the state after them.  out: n values (host), or NULL. */
int gev_glob_seeds(gev_ctx*, uint32_t* engine_state, size_t n, uint32_t* out);
/* ---- one whole generation of a randomly mating population: the body of Simulation::sim_next_generation for --RM
 * (src/Simulation.cpp:1907-1935): random_mate -> reproduce -> ras_compute_AD, enqueued as ONE unit.  Every ras_glob_seed() value
 * the three draw -- 1 (:2092) + 1 (:2398) + pop_size * nchr (:2500, only with a mutation map) -- is taken from glob_state on the
 * device, the couples never leave it, and the host waits once (in _end).
 *  glob_state            : state of glob_generator in front of random_mate's draw
 *  selection_value_func  : as gev_random_mate
 * gev_generation_end waits (enqueues the generation again with larger buffers if a list outgrew its capacity), publishes the new
 * generation and returns: res (may be NULL), the couples (pop_size records, or NULL), the offspring sexes (pop_size bytes, or
 * NULL).  gev_compute_ad then returns the generation's A/D without further device work.  Between _begin and _end no other call
 * on the context is allowed (GEV_ESTATE).  GEV_ENOMATE as gev_random_mate (nothing is published). */
typedef struct gev_generation_result {
    uint32_t glob_state;                 /* glob_generator behind the generation's last draw: the host stores it back */
    uint32_t seed_mate, seed_reproduce;  /* the values drawn at :2092 and :2398 (common_sibling needs seed_reproduce + 1, :2417) */
    uint32_t reserved;
    uint64_t num_males_mate, num_females_mate;   /* :2119-2123 */
} gev_generation_result;
int gev_generation_begin(gev_ctx*, int pop, uint32_t glob_state, size_t pop_size, const double* selection_value_func);
int gev_generation_end(gev_ctx*, gev_generation_result* res, gev_couple* couples_out, uint8_t* sex_out);
/* Head start across generations.  draws_between >= 0: the host promises that glob_generator makes exactly that many ras_glob_seed()
 * draws of its own (ras_scale_AD_compute_GEF :3078, ras_do_migration :921, ...) between the state gev_generation_end returns and the
 * state it passes to the next gev_generation_begin.  The state of the next call is then known on the device as soon as this
 * generation's seeds are drawn: the library draws the next generation's seeds and runs its sampling right away, next to this
 * generation's dense stitch, and the next gev_generation_begin (same population, same pop_size) only adds what depends on the
 * couples.  A call that arrives with another state, population or size samples again: results never depend on the promise.
 * draws_between < 0 (default): no head start. */
int gev_set_generation_chain(gev_ctx*, int draws_between);
/* ---- Simulation::ras_compute_AD + ras_find_cv (src/Simulation.cpp:2624-2815) --------------
 * additive/dominance : [n_people * nphen], index ih*nphen + iphen  (Human::additive/dominance, raw)
 * add_chr/dom_chr    : [n_people * nchr * nphen], index (ih*nchr + ichr)*nphen + iphen, or NULL
 * bv = additive + dominance is left to the host (:2715, :2744). */
int gev_compute_ad(gev_ctx*, int pop, double* additive, double* dominance,
                   double* add_chr, double* dom_chr);
/* (gev_reproduce / gev_generation_end compute the new generation's A/D with the generation, so the call after them only copies.
 * The totals of the PUBLISHED generation can also be read while the next one is in flight -- between gev_generation_begin and _end:
 * a host without selection hands the next generation over first and reads this one's values while the device works; the
 * per-chromosome arrays need the device and are refused there.) */
/* ---- Simulation::ras_scale_AD_compute_GEF (src/Simulation.cpp:3075-3206)  [SURVEY 8(f) row 1] ----
 * Scales the raw A/D of the last gev_compute_ad to the generation-0 variances, draws the noise term
 * e ~ N(0,1) from std::normal_distribution on minstd_rand0(seed) (seed = the ras_glob_seed() value
 * drawn at :3078), standardises it with CommFunc::var, and assembles phen = A + D + C + E + F.
 * The host supplies what the reference reads from host-side records: common_sibling[i]
 * (Human::common_sibling), and for gen_num > 0 the parents' values f_father[i], f_mother[i]
 * (_Pop_info_prev_gen phen or parental_effect looked up by ID_Father / ID_Mother, :3118-3131); any may be
 * NULL (= 0).  Outputs: n doubles each, any may be NULL.  Floats agree with the reference within 1e-12
 * relative (device log() and parallel sums differ from glibc / sequential sums in the last bits). */
typedef struct gev_gef_params {
    double va, vd, ve, vf, beta;        /* Phenotype_scheme::_va,_vd,_ve,_vf,_beta                        */
    double s2_a_gen0, s2_d_gen0;        /* Population::_var_a_gen0 / _var_d_gen0 of this phenotype        */
    int32_t gen_num, reserved;
} gev_gef_params;
int gev_scale_ad_compute_gef(gev_ctx*, int pop, int phen, const gev_gef_params* par, uint32_t seed,
                             const double* common_sibling, const double* f_father, const double* f_mother,
                             double* additive, double* dominance, double* bv, double* e_noise,
                             double* parental_effect, double* phen_out);
/* (the phen result of every (pop, phen) also stays in the library, [n_people x nphen] per population, for gev_compute_selection.) */

/* ---- Simulation::ras_compute_mating_value_selection_value (src/Simulation.cpp:3300-3342) + ras_selection_func (:3386-3428) ----
 * On the device, from the phenotypes the last gev_scale_ad_compute_gef of every phenotype left there, one thread per individual:
 *   mv = sum_p omega[p] * (phen[p] + shift[p]),  sv = sum_p lambda[p] * (phen[p] + shift[p])   (phenotype order, FP64, no FMA)
 *   gen_num == 0: the generation-0 mean and variance of sv (CommFunc::mean / CommFunc::var, n-1) are computed and kept for the
 *                 population, on the device (no host wait)
 *   z = (sv - mean) / sqrt(var) when var > 0, else sv - mean;  svf = ras_selection_func(z), 1 for all at generation 0
 * with the reference's arithmetic: logit y = exp(b0 + b1*z), y/(1+y) -- NaN where exp overflows, and NaN never passes r < svf (the
 * individual cannot mate); probit .5*(1+erf((z-mu)/(sqrt(2)*sigma))); stab 1/(sqrt(2*pi)*sigma)*exp(-0.5*pow((z-mu)/sigma,2)) with
 * pi = 3.1415926 (src/CommFunc.cpp:4); thr z <= thr ? p1 : 1.  Floats agree with the reference within 1e-12 relative (device libm and
 * parallel sums).
 * The three vectors (Human::mating_value, selection_value = z, selection_value_func) belong to the population's current generation:
 * they follow the individuals through gev_migrate and are dropped when the individuals change otherwise (a published generation,
 * gev_init_gen0, gev_remove_rows, gev_import_rows).  gev_generation_begin_selected / gev_random_mate_selected mate on the device's
 * selection_value_func and return GEV_ESTATE when the population has none. */
#define GEV_SEL_NONE     0   /* 1 for all (a host that passes no function)                        */
#define GEV_SEL_DEFAULT  1   /* "" : logit 0 1 (:3393-3399)                                        */
#define GEV_SEL_LOGIT    2
#define GEV_SEL_PROBIT   3
#define GEV_SEL_STAB     4
#define GEV_SEL_THR      5
typedef struct gev_selection_params {
    int32_t gen_num;          /* the reference's gen_num at :3300; generation 0 sets the standardisation */
    int32_t func;             /* GEV_SEL_NONE, GEV_SEL_DEFAULT (""), GEV_SEL_LOGIT, _PROBIT, _STAB, _THR */
    double  par1, par2;       /* _selection_func_par1/2[gen_num-1] */
    const double* omega;      /* [nphen] Phenotype_scheme::_omega */
    const double* lambda;     /* [nphen] Phenotype_scheme::_lambda */
    const double* phen_shift; /* [nphen] or NULL: the --gamma constant of this population (:3291) */
} gev_selection_params;
/* outputs: n_people doubles each (host), each may be NULL; with all three NULL the call only enqueues and returns at once.
 * GEV_ESTATE when a phenotype of the current generation has not been through gev_scale_ad_compute_gef, or gen_num > 0 without
 * generation-0 statistics (computed at gen_num 0, or set by gev_set_selection_gen0). */
int gev_compute_selection(gev_ctx*, int pop, const gev_selection_params*,
                          double* mating_value, double* selection_value, double* selection_value_func);
/* the population's current device values (as gev_compute_selection left them, or as gev_migrate moved them); GEV_ESTATE when there
 * are none.  Outputs as gev_compute_selection's; waits for the device. */
int gev_download_selection(gev_ctx*, int pop, double* mating_value, double* selection_value, double* selection_value_func);
/* Population::_gen0_SV_mean / _gen0_SV_var of `pop` (waits for the device) / set by a host that computed generation 0 itself */
int gev_get_selection_gen0(gev_ctx*, int pop, double* mean, double* var);
int gev_set_selection_gen0(gev_ctx*, int pop, double mean, double var);
/* gev_generation_begin / gev_random_mate with selection_value_func = the one gev_compute_selection left on the device: nothing is
 * uploaded and the host does not wait.  Works with the head start of gev_set_generation_chain (only the couples read it). */
int gev_generation_begin_selected(gev_ctx*, int pop, uint32_t glob_state, size_t pop_size);
int gev_random_mate_selected(gev_ctx*, int pop, uint32_t seed, size_t pop_size,
                             gev_couple* couples_out, size_t* num_males_mate, size_t* num_females_mate);

/* ---- the ID fields of class Human (src/Population.h:126-137) kept by the library ------------------------------------------------
 * gev_set_track_pedigree(ctx, 1), before any gev_init_gen0 (GEV_ESTATE after; default 0: nothing below exists and every other call
 * behaves and costs as without it): per individual the seven ids ID, ID_Father, ID_Mother, ID_Fathers_Father, ID_Fathers_Mother,
 * ID_Mothers_Father, ID_Mothers_Mother stay on the device.  Generation 0: all = i (:3037-3043).  Every published generation
 * (gev_reproduce*, gev_generation_*; host couples, random and assortative mating): one kernel beside the generation's small work
 * gathers the parents' ids through the generation's father / mother rows, ID = i_people (:2473-2479); the host waits for nothing more.
 * The ids follow the individuals through gev_migrate as the selection values do.  gev_remove_rows / gev_import_rows drop them (the
 * cross-GPU records do not carry them): gev_upload_pedigree restores them from the host's bookkeeping.
 *  ids : [n_people][7] in the order above, by position.
 * With tracking on, gev_assort_mate* / gev_generation_begin_assort* called with avoid_inbreeding and pedigree == NULL run the
 * sibling / cousin test on these ids (GEV_ESTATE while they are dropped); with tracking off that call stays GEV_EINVAL.
 * gev_download_pedigree / gev_upload_pedigree: GEV_ESTATE with tracking off or without a current generation; the download also while
 * the ids are dropped.  Both wait for the device. */
int gev_set_track_pedigree(gev_ctx*, int on);
int gev_download_pedigree(gev_ctx*, int pop, int64_t* ids);
int gev_upload_pedigree(gev_ctx*, int pop, const int64_t* ids);

/* ---- Simulation::ras_scale_AD_compute_GEF (src/Simulation.cpp:3075-3206) for EVERY phenotype of a population's current generation, from
 * state the library holds: nothing per individual crosses the boundary.  Needs gev_set_track_pedigree (GEV_ESTATE without).
 * gev_generation_phenotypes enqueues on the library's stream and returns (generation 0 waits once, for _var_a_gen0 / _var_d_gen0,
 * unless gev_set_ad_gen0 gave them); gev_phenotypes_result waits and reports.  In the reference's order:
 *  seeds     the ras_glob_seed() values are drawn on the device from glob_state: at gen_num == 0 first one per phenotype with vc > 0
 *            (:3058), then one per phenotype (:3078).  gev_phenotypes_result returns them in that order and the engine state behind
 *            them; their count is what the host promises to gev_set_generation_chain.
 *  C         gen_num > 0: default_random_engine(seed_reproduce + 1) of the generation just published, per phenotype with vc > 0 in
 *            phenotype order one normal_distribution(0, sqrt(vc)) value per couple of its couples list (inbred couples included), a fresh
 *            distribution per phenotype on the same engine, handed to every child of the couple (:2417-2429, :2481-2484).  GEV_ESTATE
 *            when the population's rows changed since the generation was published.  gen_num == 0: n_people values from an engine of
 *            its own seed per phenotype (:3053-3066).
 *  E, F0     as gev_scale_ad_compute_gef draws them (seed, seed + 1).
 *  F         gen_num > 0, vf > 0: beta * (prev[ID_Father] + prev[ID_Mother]), prev = the saved record's phen (vt_type 1) or parental_effect
 *            (vt_type 2).  The saved arrays are indexed BY ID, not by position, as the reference does (:3118-3131): after a migration
 *            the two differ.  An id at or beyond the record's length is undefined behaviour in the reference: gev_phenotypes_result
 *            returns GEV_EUNSUPPORTED and the population's phenotypes count as not computed.  GEV_ESTATE without a saved record.
 *  scaling   s_a, s_d from the host's sqrt of _var_a_gen0 / va, _var_d_gen0 / vd (A, D, G are one IEEE division of the same inputs as in
 *            gev_scale_ad_compute_gef); var(e) (two passes, n-1), s_ev and P = A + D + C + E + F on the device.
 *  var       [nphen][7]: CommFunc::var of A, D, G, C, E, F, P (:2023-2037; what "adjust beta", :648-657, needs of generation 0).
 * The seven components stay with the population ([7][n_people] per phenotype, gev_download_phenotypes) and follow gev_migrate; phen is
 * also left where gev_compute_selection reads it.  A normal stream that runs out of candidate pairs (acceptance far below pi/4) is
 * answered inside gev_phenotypes_result by running the step again with more; selection values computed meanwhile are dropped.
 * One step is outstanding per context: gev_phenotypes_result (seeds: room for 2 * nphen values) before the next gev_generation_phenotypes.
 * Floats agree with gev_scale_ad_compute_gef's within 1e-12 relative.  Locus-split contexts: gev_set_ad / gev_ad_finish_device first. */
typedef struct gev_pheno_scheme { double va, vd, vc, ve, vf, beta; } gev_pheno_scheme;   /* Phenotype_scheme; beta as adjusted by the host */
typedef struct gev_phenotypes_params { int32_t gen_num, vt_type; const gev_pheno_scheme* scheme; /* [nphen] */ } gev_phenotypes_params;
int gev_generation_phenotypes(gev_ctx*, int pop, const gev_phenotypes_params*, uint32_t glob_state);
int gev_phenotypes_result(gev_ctx*, int pop, uint32_t* glob_state_after, uint32_t* seeds, double* var /* [nphen][7] */);   /* each may be NULL */
int gev_download_phenotypes(gev_ctx*, int pop, int phen, double* out /* [7][n_people]: A D G C E F P */);
/* Population::_var_a_gen0 / _var_d_gen0 of one phenotype (:557-561): computed by the gen_num == 0 call from the raw A/D (CommFunc::var),
 * or set by a host that computed generation 0 itself */
int gev_get_ad_gen0(gev_ctx*, int pop, int phen, double* var_a, double* var_d);
int gev_set_ad_gen0(gev_ctx*, int pop, int phen, double var_a, double var_d);
/* ras_save_human_info_to_Pop_info_prev_gen (:3211-3236): device copy of the current individuals' phen (+ phen_shift[p], the --gamma
 * constant of :3292, or NULL) and parental_effect in position order; call it where the reference does, behind the migration.
 * gev_upload_prev_gen: the same record from the host, phen / parental_effect = [nphen][n] (either may be NULL = 0). */
int gev_save_prev_gen(gev_ctx*, int pop, const double* phen_shift);
int gev_upload_prev_gen(gev_ctx*, int pop, const double* phen, const double* parental_effect, size_t n);
/* test hook: short_candidates != 0 starts the normal streams of the following gev_generation_phenotypes and gev_scale_ad_compute_gef
 * calls far too short, so that the step / the call is run again; *reruns (may be NULL) = such reruns over the context's life */
int gev_dbg_phenotype_knobs(gev_ctx*, int short_candidates, unsigned long long* reruns);

/* ---- the per-generation .info text on the device ----
 * Population::ras_save_human_info (src/Population.cpp:510-568): the file's bytes for individuals [ind_begin, ind_begin + n_ind) of the
 * population's current generation; with_header != 0 puts the header line in front.  out == NULL: only *bytes_written = exact size.
 * out_bytes too small: GEV_EINVAL, *bytes_written = size needed.  Waits for the device.
 * A row holds the seven ids + 1, sex, per phenotype A D G C E F P, then MV SV SV_f, separated by one space and closed by a newline;
 * every double as printf %g prints it (6 significant digits of the exact binary value, half to even; -nan for a NaN with the sign set).
 * Rows are in position order (the order of the pedigree, phenotype and selection downloads).  The largest possible row has
 * 7*21 + 2 + (7*nphen + 3)*14 bytes, so n_ind times that (plus the header: under 128 + 56*nphen bytes) always suffices.
 * Needs pedigree tracking with the ids present, every phenotype of the current generation formed by the device's phenotype step with
 * its result taken, and selection values on the device: GEV_ESTATE otherwise, the message names what is missing.  A range beyond
 * n_people: GEV_EINVAL.  n_ind == 0: the header alone, or nothing.  The tables and buffers it uses are created by the first call.
 * At most 8 phenotypes: a block of 64 rows is staged in 16 + 64 * (largest row) bytes of on-chip memory, which must fit 64 KiB
 * (GEV_EUNSUPPORTED beyond). */
int gev_format_info_text(gev_ctx*, int pop, size_t ind_begin, size_t n_ind, int with_header,
                         char* out, size_t out_bytes, size_t* bytes_written);
/* test hooks: %g of n doubles, 16 bytes per value, NUL padded; *n_exact (may be NULL) = values that took the exact path */
int gev_dbg_format_g(gev_ctx*, const double* x, size_t n, char* out, unsigned long long* n_exact);   /* on the device */
int gev_dbg_format_g_host(const double* x, size_t n, char* out, unsigned long long* n_exact);        /* same header, host build, no device */

/* ---- the .int interval file text on the device ----
 * Simulation::ras_write_hap_to_interval_format (src/Simulation.cpp:1582-1639): after the header line
 * "h_ID chr hap st en hap_index gen0_indv root_pop" one line per part, individuals in position order, chromatid 0 then 1, parts in list
 * order (the row order of gev_download_intervals):
 *     <ID+1> <chr_label> <ihap> <st> <en> <hap_index+1> <name>.<1|2> <root_population+1>
 * every number a plain decimal (ID + 1 in the reference's unsigned arithmetic: ID = -1 prints 0), name = the .indv id of founder
 * individual hap_index / 2 of the part's ROOT population, .1 for an even hap_index and .2 for an odd one (:3031-3033).  A line has at
 * most 177 bytes.
 * gev_set_founder_names: the founder individuals' names of a ROOT population (the .indv file): name i = bytes[offsets[i] ..
 * offsets[i+1]), offsets has n_individuals + 1 entries.  Kept on the host until the first formatting call.  GEV_EUNSUPPORTED for a name
 * longer than 64 bytes (a block of 256 lines is staged in 16 + 256 * 177 bytes of on-chip memory). */
int gev_set_founder_names(gev_ctx*, int root_pop, const char* bytes, const uint32_t* offsets, size_t n_individuals);
/* the .int file's bytes for individuals [ind_begin, ind_begin + n_ind) of (pop, chr); with_header != 0 puts the header line in front.
 * out == NULL: only *bytes_written = exact size.  out_bytes too small: GEV_EINVAL, *bytes_written = size needed.  A range beyond
 * n_people: GEV_EINVAL.  n_ind == 0: the header alone, or nothing.  Waits for the device.  Goes the way of gev_download_intervals
 * (a pending order is materialised, the CSR lists are derived if need be), so it works after gev_migrate, after an import and on
 * contexts without genotype planes.  Concatenating the texts of consecutive ranges, the header on the first only, gives the file.
 * ids: Human::ID of the n_ind individuals (host memory), or NULL = the ID plane the library tracks (gev_set_track_pedigree).
 * GEV_ESTATE, the message naming what is missing: interval tracking off; names of some root population of the context never set;
 * ids == NULL without pedigree tracking or with the ids dropped.  GEV_EINVAL and no text: a part whose hap_index / 2 lies beyond its
 * root population's names.  The device tables and buffers are created by the first call.  The text leaves the device in runs of
 * blocks of 256 lines (gev_dbg_output_chunk caps the blocks of a run). */
int gev_format_interval_text(gev_ctx*, int pop, int chr, int chr_label, size_t ind_begin, size_t n_ind, int with_header,
                             const int64_t* ids, char* out, size_t out_bytes, size_t* bytes_written);
/* the same header's host build from plain arrays, no device, no context: parts / hap_offsets as gev_download_intervals returns them
 * (hap_offsets + 2 * i and ids + i give the text from individual i on), names of root population p = name_bytes[p], name_offsets[p]
 * (n_names[p] + 1 entries).  Same size query and short-buffer convention; GEV_EINVAL for a part without a name. */
int gev_dbg_format_interval_text_host(const gev_part* parts, const uint64_t* hap_offsets, size_t n_ind, const int64_t* ids, int chr_label,
                                      const char* const* name_bytes, const uint32_t* const* name_offsets, const size_t* n_names, int n_root_pop,
                                      int with_header, char* out, size_t out_bytes, size_t* bytes_written);

/* ---- Simulation::assort_mate (src/Simulation.cpp:2167-2360), the reference's default mating mode -------------------------------
 * Forms the couples of the population's current generation on the device, bit for bit as the reference does (stable order among
 * equal mating values, as the host mirror geneevolve_amd/host.py:assort_mate; std::sort leaves it unspecified):
 *  seeds[4]             : the ras_glob_seed() values drawn at :2170 (srand), :2173 (selection generator), :2265 (ras_mvnorm) and,
 *                         with offspring_dist 'p' only, :2332 (ras_rpois)
 *  mating_value         : Human::mating_value [n_people] (:2251)
 *  selection_value_func : [n_people] (:2190), or NULL when every value is 1; NaN never passes
 *  pedigree             : [n_people][5] ids (ID_Father, ID_Fathers_Father, ID_Fathers_Mother, ID_Mothers_Father, ID_Mothers_Mother)
 *                         for the sibling / cousin test of avoid_inbreeding (:2306-2322); NULL without it, or to use the ids the
 *                         library tracks (gev_set_track_pedigree)
 *  couples_out          : res->n_couples records, or NULL (size it from a call with NULL first, or from an upper bound:
 *                         n_couples <= n_people)
 * Second spouses (--MM, :2196-2198), surplus removal by std::random_shuffle on glibc rand() (:2232-2246), the ras_mvnorm rank
 * template (:2257-2285), inbreeding avoidance and the offspring numbers ('p': poisson_distribution, mean < 12; 'f': pop_size /
 * couples each, the remainder to the first couples of a shuffled list, :2328-2355) all run on the device.  Device log() may differ
 * from glibc's in the last bit: a couple can change only where two template values lie within a few ulp of each other.
 * The couples stay on the device: the next gev_reproduce of `pop` with couples == NULL and n_people == res->n_offspring breeds from
 * them (same GEV_ESTATE rule as after gev_random_mate).
 * Errors: GEV_ENOMATE "Error: couples=0, ..." (:2226-2230); GEV_EUNSUPPORTED for a Poisson mean >= 12, for no couple left after
 * the inbred ones, and for avoid_inbreeding with 'f' and a remainder (the reference indexes an empty vector there); GEV_EINVAL for
 * another offspring_dist, a non-finite mat_cor or a NULL pedigree with avoid_inbreeding on a context that does not track the ids. */
typedef struct gev_assort_params {
    uint64_t pop_size;          /* --pop_size of the next generation */
    double   mat_cor;           /* mating-value correlation of spouses */
    double   mm_percent;        /* --MM: probability of a second spouse */
    int32_t  avoid_inbreeding;  /* --avoid_inbreeding */
    int32_t  offspring_dist;    /* 'p' / 'P' or 'f' / 'F' */
} gev_assort_params;
typedef struct gev_assort_result {
    uint64_t num_males_mate, num_females_mate;   /* list lengths before the surplus removal, second spouses included (:2222-2223) */
    uint64_t n_couples, n_inbreed, n_offspring;  /* couples formed, inbred ones among them, children of the others */
} gev_assort_result;
int gev_assort_mate(gev_ctx*, int pop, const gev_assort_params*, const uint32_t seeds[4], const double* mating_value,
                    const double* selection_value_func, const int64_t* pedigree, gev_couple* couples_out, gev_assort_result* res);
/* gev_assort_mate on the mating values and selection_value_func gev_compute_selection left on the device (GEV_ESTATE without) */
int gev_assort_mate_selected(gev_ctx*, int pop, const gev_assort_params*, const uint32_t seeds[4], const int64_t* pedigree,
                             gev_couple* couples_out, gev_assort_result* res);
/* the result of the last gev_assort_mate(_selected) of the context (also of a gev_generation_begin_assort in flight: allowed between
 * _begin and _end); its couples as records when couples_out is not NULL (res->n_couples of them; not between _begin and _end) */
int gev_last_assort_result(gev_ctx*, gev_assort_result* res, gev_couple* couples_out);
/* ---- one whole assortative generation: the body of Simulation::sim_next_generation without --RM (src/Simulation.cpp:1907-1935):
 * assort_mate -> reproduce -> ras_compute_AD as one call pair, finished by gev_generation_end.  Every ras_glob_seed() value of the
 * generation -- 3 (:2170, :2173, :2265), a 4th with 'p' (:2332), then 1 (:2398) + n_offspring * nchr (:2500, only with a mutation
 * map) -- is drawn on the device from glob_state; res->glob_state of gev_generation_end is the state behind the last one, res->seed_mate
 * the srand seed (:2170), res->num_*_mate the list lengths.  Begin waits internally for the mating counts (n_offspring is random under
 * 'p'); the rest of the generation is enqueued as gev_generation_begin's and _end waits once.  gev_last_assort_result (between _begin
 * and _end) sizes the outputs of gev_generation_end: couples_out holds n_couples records, sex_out n_offspring bytes.
 * The head start of gev_set_generation_chain does not apply: a head start queued by a random-mating generation is dropped here, and
 * none is queued behind an assortative generation.  Arguments and errors as gev_assort_mate (nothing pending after an error). */
int gev_generation_begin_assort(gev_ctx*, int pop, uint32_t glob_state, const gev_assort_params*, const double* mating_value,
                                const double* selection_value_func, const int64_t* pedigree);
int gev_generation_begin_assort_selected(gev_ctx*, int pop, uint32_t glob_state, const gev_assort_params*, const int64_t* pedigree);
/* test hooks of the exact fallbacks, in force for the following calls: narrow_window != 0 shrinks the windows of the marriage-draw chain
 * so that most chunks are walked directly; short_poisson != 0 starts the Poisson stream far too short so that it is extended and run
 * again.  gev_dbg_assort_stats: {chunks, chunks walked directly, Poisson reruns} of the last gev_assort_mate. */
int gev_dbg_assort_knobs(gev_ctx*, int narrow_window, int short_poisson);
int gev_dbg_assort_stats(gev_ctx*, unsigned long long stats[3]);

/* Locus-split populations (gev_set_chr_active): every context of the population computes the A/D of its own chromosomes; after
 * the all-reduce + chromosome-ordered sum (geneevolve_amd/distributed.py:compute_ad_locus_split) each context is handed the raw
 * totals [n_people * nphen] of the current generation, which is what gev_scale_ad_compute_gef scales (:3104-3105). */
int gev_set_ad(gev_ctx*, int pop, const double* additive, const double* dominance);

/* population allele frequency frq[icv] of the last gev_compute_ad (:2647-2655), FILE order. */
int gev_get_cv_freq(gev_ctx*, int pop, int phen, int chr, double* frq, size_t C);

/* ---- Simulation::ras_do_migration (src/Simulation.cpp:877-989) ----------------------------
 * The host decides WHO moves exactly as the reference does; the library moves the rows:
 * migrants are removed from their origin populations (stable order of the remainder, :960-966)
 * and appended to their destinations in `moves` order (:971-981). */
int gev_migrate(gev_ctx*, const gev_move* moves, size_t n_moves);
/* Cross-GPU form of the same step (one context per GPU, exchange done by the caller over
 * RCCL): pack the complete state of the individuals at `positions` into one contiguous device
 * buffer / remove them / append individuals packed by a peer.  Record layout is opaque but
 * identical across contexts with identical static inputs; gev_export_size gives the byte count. */
int gev_export_size(gev_ctx*, int pop, const uint64_t* positions, size_t n, size_t* bytes);
int gev_export_rows(gev_ctx*, int pop, const uint64_t* positions, size_t n, void* device_buf, size_t bytes);
int gev_remove_rows(gev_ctx*, int pop, const uint64_t* positions, size_t n);
int gev_import_rows(gev_ctx*, int pop, const void* device_buf, size_t bytes, size_t n);
/* Migrants that travel as lists.  A migrant's genotype row is redundant with what travels beside it: it is the founder mosaic its
 * ancestry intervals describe -- out[ii] = pops[part.root_population].hap_snps[part.hap_index][ii] for the part that contains
 * pos[ii], Simulation::ras_convert_interval_to_hap_matrix (src/Simulation.cpp:1198-1211) -- with the mutations kept beside it as
 * a sparse list.  A context that holds the founder panels of the root populations (read-only copies: what the reference keeps
 * as Population::hap_snps for the whole run, src/Population.h) can therefore rebuild the rows where they arrive:
 *  gev_upload_founder_panel / gev_synth_founder_panel : Hap_SNP.hap of ROOT population `pop`, chromosome chr, kept for good
 *                            (same arguments as gev_upload_founders / gev_synth_founders; `pop` need not be simulated here;
 *                            gev_set_snps of (pop, chr) first).  Needs resident planes (not gev_set_dense_state 0).
 *  gev_set_migrant_rows(0) : gev_export_size / gev_export_rows leave the genotype rows out of the records (sexes, CV rows, mutation
 *                            and interval lists travel as before), gev_import_rows assembles the immigrants' rows from the
 *                            panels.  Needs the interval state (gev_set_track_intervals 1).  Both ends of an exchange use the
 *                            same setting; gev_import_rows returns GEV_ESTATE when an immigrant descends from a root population
 *                            without a panel here, GEV_EINVAL with the reference's "p.hap_index is not in range" (:1205-1209).
 * At BASELINE config 2's shape a migrant is 250 KB of rows against 0.2-20 KB of lists. */
int gev_upload_founder_panel(gev_ctx*, int pop, int chr, const uint64_t* bits, size_t row_stride_words, size_t nhap, size_t L);
int gev_synth_founder_panel(gev_ctx*, int pop, int chr, size_t nhap, uint64_t seed);
int gev_set_migrant_rows(gev_ctx*, int on);

/* ---- output materialisation --------------------------------------------------------------
 * == Simulation::ras_convert_interval_to_hap_matrix (src/Simulation.cpp:1186-1230):
 * rows [row_begin, row_begin+n_rows) of the 2*n_people x L matrix, mutations applied. */
int gev_download_haps(gev_ctx*, int pop, int chr, size_t row_begin, size_t n_rows,
                      uint64_t* bits, size_t row_stride_words);
int gev_materialize_pops(gev_ctx*, int pop, int chr, size_t row_begin, size_t n_rows, size_t snp_begin, size_t n_snps,
                         const uint64_t* const* founder_bits, const size_t* founder_stride_words, const size_t* n_founder_rows,
                         uint64_t* bits, size_t row_stride_words);
/* PLINK .bed body (as gev_format_bed) of SNPs [snp_begin, +n_snps) assembled from the interval state + founder tiles: the output
 * path of plane-less contexts (BASELINE config 5: "PLINK bit-packed output"); n_snps * ceil(n_people/4) bytes. */
int gev_materialize_bed(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps,
                        const uint64_t* const* founder_bits, const size_t* founder_stride_words, const size_t* n_founder_rows,
                        uint8_t* out, size_t out_bytes);
/* ---- K9 output packing [SURVEY 8(f) row 3]: SNP-major forms of the same matrix, built on the device
 * (64x64 bit-tile transposes + mutation overlay).
 *  gev_download_snp_major : row = SNP (snp_begin + j), bit h = haplotype row h; ceil(2*n_people/64) words per row
 *  gev_format_hap_text    : the exact bytes format_hap::write_hap (src/format_hap.cpp:6-30) writes for these SNP
 *                           lines: per line "b b ... b \n", i.e. n_snps * (4*n_people + 1) bytes
 *  gev_format_bed         : PLINK .bed body (SNP-major, 2 bits / individual, A1 = allele 1: 00 = 1/1, 10 = het,
 *                           11 = 0/0, pad 00; without the 3 magic bytes): n_snps * ceil(n_people/4) bytes.  The
 *                           reference has no .bed writer (BASELINE config 5 asks for one): checked by definition.
 *  gev_format_vcf_gt      : the sample columns format_vcf::write_vcf_file (src/format_vcf.cpp:55-59) appends to each data
 *                           line: per individual "\ta|b", then '\n' = n_snps * (4*n_people + 1) bytes; the nine fixed
 *                           columns (CHROM..FORMAT, host strings of the input VCF) are the caller's.  Pinned on the
 *                           reference's own .vcf output (fixture `dense`; the reference's VCF-panel path needs the one
 *                           missing `return` of format_vcf.cpp:367-389 supplied, see oracle/ref_vcf_return.cpp). */
int gev_download_snp_major(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, uint64_t* bits, size_t row_stride_words);
int gev_format_hap_text(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, char* out, size_t out_bytes);
int gev_format_bed(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, uint8_t* out, size_t out_bytes);
int gev_format_vcf_gt(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, char* out, size_t out_bytes);
/* ---- genotype counts per SNP: allele frequencies and heterozygosity without a dump -------------------------------------------
 * per SNP of [snp_begin, +n_snps), over individuals [ind_begin, +n_ind) of the current generation, new mutations applied:
 *   n_het[j]     = individuals whose two haplotypes differ at SNP snp_begin+j
 *   n_hom_alt[j] = individuals with allele 1 on both
 * (alt allele count = n_het + 2*n_hom_alt; hom-ref = n_ind - n_het - n_hom_alt).  Counted on the device from the resident rows where
 * they lie (a positional popcount over the haplotype-major planes plus a sparse correction from the mutation lists: no transpose, no
 * staging copy, two vectors of n_snps counts come back); rows 2i and 2i+1 are individual i's haplotypes.  Begins like the other
 * output calls: a pending order (gev_migrate) is materialised, the planes are waited for.  GEV_ESTATE on a context without genotype
 * planes (gev_set_dense_state 0), for an inactive chromosome and for a population without a current generation; GEV_EINVAL for a range
 * beyond L / n_people and for a NULL vector with n_snps > 0.  n_snps == 0 touches nothing, n_ind == 0 writes zeros.  Returns when both
 * vectors are in the caller's memory.  The device vectors are created by the first call. */
int gev_snp_genotype_counts(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind,
                            uint32_t* n_het, uint32_t* n_hom_alt);
/* the same counter (csrc/gev_snpcount.h) built for the host, on haplotype-major rows in host memory as gev_download_haps returns them
 * (rows 2i, 2i+1 = individual i, row_stride_words >= ceil(L/64)), over all n_ind individuals: no device, no context.  Words of a row
 * that hold no SNP of the range are not read. */
int gev_dbg_snp_counts_host(const uint64_t* bits, size_t row_stride_words, size_t n_ind, size_t L,
                            size_t snp_begin, size_t n_snps, uint32_t* n_het, uint32_t* n_hom_alt);
/* ---- genotype counts per individual and per pair of individuals: kinship, IBS and GRM without a dump -----------------------------
 * Counted on the device from the resident rows of the current generation, new mutations applied (csrc/gev_paircount.h): each side's
 * rows are staged once, one pass makes the range-masked planes x = a ^ b and y = a & b and the per-individual counts, and the pair
 * counts are two exact integer matrix products on the matrix cores (v_mfma_i32_16x16x64_i8) finished in the same kernel.  Counts are
 * additive over SNP ranges and over chromosomes: one call serves one (pop, chr).  Both calls begin like the other output calls (a
 * pending order is materialised, the planes are waited for) and return when the results are in the caller's memory.  GEV_ESTATE on a
 * context without genotype planes, for an inactive chromosome and for a population without a current generation; GEV_EINVAL for a
 * range beyond L / n_people; GEV_EUNSUPPORTED for n_snps > 2^30 (dot can reach 4 * n_snps).  The device buffers are created by the
 * first call; gev_dbg_output_chunk caps the individuals of one staging pass (and so the side of a sub-block of the pair matrix).
 *
 * per individual of [ind_begin,+n_ind), over SNPs [snp_begin,+n_snps) of (pop, chr):
 *   n_het[i], n_hom_alt[i]   uint32;
 *   wsum[i] = sum_j weight[j] * g_ij (uint64; g = 0/1/2 copies of allele 1; weight: n_snps uint32 in host memory)
 *   weight == NULL <=> wsum == NULL (GEV_EINVAL otherwise); each output may be NULL.  n_snps == 0 writes zeros, n_ind == 0 touches nothing */
int gev_ind_genotype_counts(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind,
                            const uint32_t* weight, uint32_t* n_het, uint32_t* n_hom_alt, uint64_t* wsum);
/* for every pair (i of [a_begin,+n_a), k of [b_begin,+n_b)) of one population, row-major [n_a][n_b] uint32, each may be NULL:
 *   n_hethet  loci where both are heterozygous
 *   n_opphom  loci where one is 0/0 and the other 1/1 (IBS0)
 *   dot       sum_j g_ij * g_kj
 * n_snps == 0 writes zeros; n_a == 0 or n_b == 0 touches nothing */
int gev_pair_genotype_counts(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps,
                             size_t a_begin, size_t n_a, size_t b_begin, size_t n_b,
                             uint32_t* n_hethet, uint32_t* n_opphom, uint32_t* dot);
/* the same arithmetic (masking, expansion of bits to operand bytes, finishing formulas) compiled for the host on rows in host memory
 * as gev_download_haps returns them (rows 2i, 2i+1 = individual i, row_stride_words >= ceil(L/64)), a plain integer loop in place of
 * the matrix instruction: no device, no context.  n_het / n_hom_alt: all n_ind individuals; the pair ranges lie in [0, n_ind).  Words
 * of a row that hold no SNP of the range are not read. */
int gev_dbg_pair_counts_host(const uint64_t* bits, size_t row_stride_words, size_t n_ind, size_t L, size_t snp_begin, size_t n_snps,
                             size_t a_begin, size_t n_a, size_t b_begin, size_t n_b,
                             uint32_t* n_het /*[n_ind]*/, uint32_t* n_hom_alt /*[n_ind]*/,
                             uint32_t* n_hethet, uint32_t* n_opphom, uint32_t* dot);
/* ---- linkage disequilibrium per pair of SNPs: r^2 blocks and LD scores without a dump ----------------------------------------------
 * Counted on the device from the current generation, new mutations applied (csrc/gev_ldcount.h): a side's SNPs are turned SNP-major
 * (row = SNP, bit h = haplotype row h, bits 2i and 2i+1 = individual i), one pass cuts the rows to the haplotypes of individuals
 * [ind_begin, +n_ind), writes the side's plane and counts per SNP, and the pair counts are exact integer matrix products on the matrix
 * cores (v_mfma_i32_16x16x64_i8) over n = 2 n_ind haplotypes (n11) and N = n_ind individuals (gg).  Both calls begin like the other
 * output calls (a pending order is materialised, the planes are waited for) and return when the results are in the caller's memory.
 * GEV_ESTATE on a context without genotype planes, for an inactive chromosome and for a population without a current generation;
 * GEV_EINVAL for a range beyond L / n_people; GEV_EUNSUPPORTED for n_ind > 2^30.  The device buffers are created by the first call;
 * gev_dbg_output_chunk caps the SNPs of one SNP-major pass and the side of a sub-block of the SNP-pair matrix.
 *
 * gev_ld_counts: for SNP j of [a_begin,+n_a) of chr_a and SNP k of [b_begin,+n_b) of chr_b (chr_a != chr_b is allowed: the
 * disequilibrium between chromosomes), row-major [n_a][n_b] uint32, each may be NULL:
 *   n11   haplotypes of the range that carry allele 1 at both SNPs
 *   gg    sum over the individuals of the range of g_ij * g_ik (g = 0/1/2 copies of allele 1)
 * and per SNP of each side over the same individuals, uint32 [n_a] / [n_b], each may be NULL:
 *   c (allele-1 count = sum g), n_het, n_hom_alt (sum g^2 = n_het + 4 n_hom_alt)
 * n_ind == 0 writes zeros; n_a == 0 or n_b == 0 touches nothing.
 * Haplotype r^2 = (n n11 - c_j c_k)^2 / (c_j (n - c_j) c_k (n - c_k)); genotype r^2 = (N gg - s_j s_k)^2 / ((N sum g_j^2 - s_j^2)(..k..)). */
int gev_ld_counts(gev_ctx*, int pop, int chr_a, size_t a_begin, size_t n_a, int chr_b, size_t b_begin, size_t n_b, size_t ind_begin, size_t n_ind,
                  uint32_t* n11, uint32_t* gg, uint32_t* c_a, uint32_t* het_a, uint32_t* hom_a, uint32_t* c_b, uint32_t* het_b, uint32_t* hom_b);
/* gev_ld_scores: for SNP j = snp_begin + t of [snp_begin,+n_snps) the window is SNPs [win_lo[t], win_hi[t]) of the same chromosome
 * (host arrays of n_snps uint32, both non-decreasing, win_lo[t] <= j < win_hi[t] <= L; GEV_EINVAL otherwise; windows may reach outside
 * the range of the call).  genotype: 0 haplotype r^2, otherwise genotype r^2.  Each output may be NULL:
 *   score_q40[t] (uint64) = sum over the window, j itself included, of the r^2 quantum llrint(r^2 * 2^40), r^2 formed in separately
 *                rounded IEEE double operations from the exact integers (num^2 / (den_j den_k)); 0 where either SNP is monomorphic
 *                among the individuals (den = 0).  The sum is an integer sum: the same on every run and in every order.
 *   n_terms[t]   (uint32) = the window's SNPs with den > 0
 * The band is walked on the device and reduced there; no pair matrix is written or copied out.  n_snps == 0 touches nothing,
 * n_ind == 0 writes zeros. */
int gev_ld_scores(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, const uint32_t* win_lo, const uint32_t* win_hi,
                  size_t ind_begin, size_t n_ind, int genotype, uint64_t* score_q40, uint32_t* n_terms);
/* the same arithmetic (masking, expansion of bits to operand bytes, counts, quantum) compiled for the host on rows in host memory as
 * gev_download_haps returns them (2 n_people rows, rows 2i, 2i+1 = individual i, stride >= ceil(L/64) words), a plain integer loop in
 * place of the matrix instruction: no device, no context.  The block form as gev_ld_counts (bits_b may be bits_a, or another
 * chromosome's rows of the same people); with win_lo / win_hi the score form as gev_ld_scores over SNPs [a_begin,+n_a) of bits_a.
 * Only the rows of the individuals of the range are read, and of those the words that hold a SNP of a side or a window. */
int gev_dbg_ld_host(const uint64_t* bits_a, size_t stride_a, size_t L_a, const uint64_t* bits_b, size_t stride_b, size_t L_b, size_t n_people,
                    size_t a_begin, size_t n_a, size_t b_begin, size_t n_b, size_t ind_begin, size_t n_ind,
                    uint32_t* n11, uint32_t* gg, uint32_t* c_a, uint32_t* het_a, uint32_t* hom_a, uint32_t* c_b, uint32_t* het_b, uint32_t* hom_b,
                    const uint32_t* win_lo, const uint32_t* win_hi, int genotype, uint64_t* score_q40, uint32_t* n_terms);
/* the r^2 quantum alone (gev_ld_r2_q40 of csrc/gev_ldcount.h compiled for the host) on n triples with num^2 <= den_j * den_k, as the
 * counts of real data always have it (Cauchy-Schwarz): q40[i] = llrint(((double)num * (double)num) / ((double)den_j * (double)den_k) * 2^40),
 * 0 where a denominator is 0 */
int gev_dbg_ld_r2_q40_host(const int64_t* num, const uint64_t* den_j, const uint64_t* den_k, size_t n, uint64_t* q40);
/* ---- trait sums per SNP: an association scan without a dump -------------------------------------------------------------------------
 * Counted on the device from the current generation, new mutations applied (csrc/gev_traitsum.h).  A trait is a host vector of int32
 * quanta q[t][i], |q| <= 2^30, entry i = individual ind_begin + i (floating-point phenotypes are quantised by the caller:
 * geneevolve_amd/assoc.py), so every sum is an exact integer sum, the same on every run and in every order.  For SNP j of
 * [snp_begin,+n_snps) and trait t over individuals [ind_begin,+n_ind), each output may be NULL:
 *   gsum[t][j]   (int64, [n_traits][n_snps]) = sum_i g_ij q[t][i], g = 0/1/2 copies of allele 1
 *   hetsum[t][j] (int64, [n_traits][n_snps]) = sum of q[t][i] over the individuals heterozygous at j
 *   n_het[j], n_hom_alt[j] (uint32 [n_snps]) = the heterozygous / homozygous-alt individuals, as gev_ld_counts gives them
 * The genotype-class sums are S1 = hetsum and S2 = (gsum - hetsum) / 2; S0 follows from sum q, which the caller owns.  The SNPs go
 * through the SNP-major pass and the plane of gev_ld_counts; the quanta are split into four balanced base-256 digits, and the sums
 * are integer matrix products on the matrix cores (v_mfma_i32_16x16x64_i8) with the individuals split over workgroups.  The call
 * begins like the other output calls and returns when the results are in the caller's memory.  GEV_ESTATE on a context without
 * genotype planes, for an inactive chromosome and for a population without a current generation; GEV_EINVAL for a range beyond L /
 * n_people, for a NULL trait with n_traits > 0 and n_ind > 0 and for a quantum beyond +-2^30 (checked before anything is enqueued);
 * GEV_EUNSUPPORTED for n_ind > 2^22 (a digit's sum is an int32).  n_snps == 0 touches nothing, n_ind == 0 writes zeros, n_traits == 0
 * gives the two count vectors only.  The device buffers are created by the first call; gev_dbg_output_chunk caps the SNPs of one pass. */
int gev_snp_trait_sums(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind,
                       const int32_t* trait /*[n_traits][n_ind], host*/, size_t n_traits,
                       int64_t* gsum /*[n_traits][n_snps]*/, int64_t* hetsum /*[n_traits][n_snps]*/,
                       uint32_t* n_het /*[n_snps]*/, uint32_t* n_hom_alt /*[n_snps]*/);
/* the same arithmetic (masking, digit split, byte order of both operands, recombination) compiled for the host on rows in host memory
 * as gev_download_haps returns them (2 n_people rows, stride >= ceil(L/64) words), a plain integer loop in place of the matrix
 * instruction: no device, no context.  Only the rows of the individuals of the range are read, and of those the words that hold a SNP
 * of the range. */
int gev_dbg_trait_sums_host(const uint64_t* bits, size_t row_stride_words, size_t n_people, size_t L, size_t snp_begin, size_t n_snps,
                            size_t ind_begin, size_t n_ind, const int32_t* trait, size_t n_traits,
                            int64_t* gsum, int64_t* hetsum, uint32_t* n_het, uint32_t* n_hom_alt);
/* ---- scores per individual: polygenic scores with signed weight columns without a dump ----------------------------------------------
 * Counted on the device from the resident rows of the current generation, new mutations applied (csrc/gev_indscore.h).  A score column
 * is a host vector of int32 weights w[s][j], |w| <= 2^30, entry j = SNP snp_begin + j (floating-point effect sizes are quantised by the
 * caller: geneevolve_amd/scores.py), so every sum is an exact integer sum, the same on every run and in every order, and additive over
 * SNP ranges and chromosomes: one call serves one (pop, chr).  For individual i of [ind_begin,+n_ind) and column s over SNPs
 * [snp_begin,+n_snps), each output may be NULL:
 *   gscore[s][i]   (int64, [n_scores][n_ind]) = sum_j w[s][j] g_ij, g = 0/1/2 copies of allele 1; |gscore| <= 2^53
 *   hetscore[s][i] (int64, [n_scores][n_ind]) = sum of w[s][j] over the SNPs at which i is heterozygous
 * The genotype-class sums are S1 = hetscore and S2 = (gscore - hetscore) / 2.  The individuals go through the staging pass and the
 * planes x = a ^ b, y = a & b of gev_pair_genotype_counts; the weights are split into four balanced base-256 digits, and the sums are
 * integer matrix products on the matrix cores (v_mfma_i32_16x16x64_i8) with the SNPs split over workgroups.  The call begins like the
 * other output calls and returns when the results are in the caller's memory.  GEV_ESTATE on a context without genotype planes, for
 * an inactive chromosome and for a population without a current generation; GEV_EINVAL for a range beyond L / n_people, for a NULL
 * weight with n_scores > 0 and n_snps > 0 and for a weight beyond +-2^30 (checked before anything is enqueued); GEV_EUNSUPPORTED for
 * n_snps > 2^22 (a digit's sum is an int32; the caller splits the range and adds).  n_ind == 0 touches nothing, n_snps == 0 or
 * n_scores == 0 writes zeros.  The device buffers are created by the first call; gev_dbg_output_chunk caps the individuals of one
 * staging pass and of one block. */
int gev_ind_scores(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind,
                   const int32_t* weight /*[n_scores][n_snps], host*/, size_t n_scores,
                   int64_t* gscore /*[n_scores][n_ind]*/, int64_t* hetscore /*[n_scores][n_ind]*/);
/* the same arithmetic (masking, digit split, byte order of both operands, recombination) compiled for the host on rows in host memory
 * as gev_download_haps returns them (2 n_people rows, stride >= ceil(L/64) words), a plain integer loop in place of the matrix
 * instruction: no device, no context.  Only the rows of the individuals of the range are read, and of those the words that hold a SNP
 * of the range. */
int gev_dbg_ind_scores_host(const uint64_t* bits, size_t row_stride_words, size_t n_people, size_t L, size_t snp_begin, size_t n_snps,
                            size_t ind_begin, size_t n_ind, const int32_t* weight, size_t n_scores, int64_t* gscore, int64_t* hetscore);
/* ---- identity by descent per pair of haplotypes, from the ancestry intervals: realised coancestry and inbreeding without a dump ------
 * The one analysis call on the interval lists (csrc/gev_ibd.h).  For haplotype row r (row = 2 * individual + chromatid) of (pop, chr)
 * let f_r(x) = (root_population, hap_index) of the part of r's list with st <= x < en (half-open, as part::check_interval, reference
 * src/Population.h), undefined where no part covers x.  The IBD set of rows r, s is {x : f_r(x) and f_s(x) defined and equal}; its
 * segments are its maximal intervals (a segment runs on where both rows change founder together and still agree, and across adjacent
 * parts of one row with the same label).  New mutations play no part: this is identity by founder origin.  Over the segments of length
 * >= min_bp (0: all of them), for row a_begin + i of pop_a against row b_begin + k of pop_b (the same population or another one; the
 * ranges may overlap, coincide or be disjoint), row-major [n_a][n_b], each may be NULL:
 *   shared_bp (uint64)  the summed length of the segments
 *   n_seg     (uint32)  their number
 *   max_seg   (uint64)  the longest, 0 without one
 * Plain 64-bit integers: exact and the same on every run.  One workgroup takes a tile of 16 x 16 pairs, one pair per lane, each lane
 * walking its two lists with two cursors where they lie.  Nothing bounds a row's length; rows without parts share nothing.  The call begins like gev_format_interval_text, for both
 * populations (a pending order is materialised, the CSR lists are derived if need be), so it works after gev_migrate, after an import
 * and on contexts without genotype planes (gev_set_dense_state 0), and returns when the results are in the caller's memory.
 * GEV_ESTATE, the message naming what is missing: interval tracking off, an inactive chromosome, a population without a current
 * generation, a generation pending; GEV_EINVAL for a range beyond 2 * n_people.  n_a == 0 or n_b == 0 touches nothing.  The device
 * buffers are created by the first call; the results leave in sub-blocks of at most 4096 rows a side (gev_dbg_output_chunk caps them). */
int gev_ibd_sharing(gev_ctx*, int chr, int pop_a, size_t a_begin, size_t n_a, int pop_b, size_t b_begin, size_t n_b,
                    uint64_t min_bp, uint64_t* shared_bp, uint32_t* n_seg, uint64_t* max_seg);
/* per haplotype row of [row_begin, +n_rows) of (pop, chr), one thread per row, each may be NULL:
 *   bp[r][p]   (uint64 [n_rows][n_pop]) the base pairs of the row covered by parts whose root_population is p: local-ancestry totals,
 *              admixture proportions after migration
 *   n_parts[r] (uint32 [n_rows]) the length of the row's list
 * Begins as gev_ibd_sharing and returns the same errors; a root_population outside [0, n_pop): GEV_EINVAL, nothing is written.
 * n_rows == 0 touches nothing. */
int gev_ancestry_bp(gev_ctx*, int pop, int chr, size_t row_begin, size_t n_rows,
                    uint64_t* bp /* [n_rows][n_pop] */, uint32_t* n_parts /* [n_rows] */);
/* the same walk (csrc/gev_ibd.h) compiled for the host on lists in host memory as gev_download_intervals returns them (parts of row r of
 * side a = parts_a[off_a[r] .. off_a[r+1]), off_* has n_* + 1 entries; parts of a row in position order, not overlapping): no device, no
 * context.  Outputs as gev_ibd_sharing's. */
int gev_dbg_ibd_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b,
                     uint64_t min_bp, uint64_t* shared_bp, uint32_t* n_seg, uint64_t* max_seg);
/* ---- the IBD segments themselves: where the tracts two haplotypes share lie on the chromosome -------------------------------------
 * One record per segment of length >= min_bp of the definition above (a maximal interval of the IBD set of two rows: it runs on across
 * a common change of founder and across adjacent same-label parts of one row; new mutations play no part), [st, en) half-open, for
 * row a_begin + i of pop_a against row b_begin + k of pop_b.  row_a / row_b are the absolute rows in their populations
 * (2 * individual + chromatid).  pairs: GEV_IBD_ALL_PAIRS, or GEV_IBD_UPPER for the pairs with row_a < row_b alone, which takes one
 * population (pop_a == pop_b; GEV_EINVAL otherwise; the ranges may differ).  The records come sorted by (row_a, row_b, st), whatever
 * the strips, tiles and gev_dbg_output_chunk were: the list is the same bytes on every run.
 *   *n_total is always set to the number of records of the request (n_total == NULL: GEV_EINVAL).  out is filled if and only if
 *   *n_total <= capacity; otherwise the call still returns GEV_OK, the caller sees *n_total > capacity and nothing of out is written
 *   (never a byte at or beyond out[capacity]).  out == NULL with capacity == 0 is the count-only form; a call with the counted capacity
 *   then fills.  n_a == 0 or n_b == 0 sets *n_total = 0 and touches nothing else.
 * The pair matrix is walked in strips of whole A rows against all n_b B rows (at most 2^24 pairs, at least one row;
 * gev_dbg_output_chunk caps a strip's A rows; a strip of more than 1 GiB of records is halved in rows until it fits or is one row): a
 * count kernel, and when out fits an exclusive scan and a fill kernel that walks again, each lane writing its pair's records from the
 * pair's offset into a device buffer that is copied to out at the strip's running offset.  So an out that fits costs two walks, three
 * when the request is more than one strip.  Begins as gev_ibd_sharing, for both populations, and returns its errors; a row index that
 * does not fit 32 bits, or a single row with 2^32 records or more: GEV_EUNSUPPORTED.  A refused call leaves out and *n_total as they
 * were.  The device buffers are created by the first call. */
typedef struct gev_ibd_segment { uint64_t st, en; uint32_t row_a, row_b; } gev_ibd_segment;   /* 24 bytes, [st, en) */
#define GEV_IBD_ALL_PAIRS 0
#define GEV_IBD_UPPER     1
int gev_ibd_segments(gev_ctx*, int chr, int pop_a, size_t a_begin, size_t n_a, int pop_b, size_t b_begin, size_t n_b,
                     uint64_t min_bp, int pairs, gev_ibd_segment* out, size_t capacity, uint64_t* n_total);
/* the same walk compiled for the host on lists in host memory, as gev_dbg_ibd_host takes them and with its refusals: no device, no
 * context.  row_a / row_b are indices into off_a / off_b; GEV_IBD_UPPER takes the same lists on both sides (parts_a == parts_b and
 * off_a == off_b; n_a and n_b may differ).  out, capacity and n_total as above. */
int gev_dbg_ibd_segments_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a, const gev_part* parts_b, const uint64_t* off_b, size_t n_b,
                              uint64_t min_bp, int pairs, gev_ibd_segment* out, size_t capacity, uint64_t* n_total);
/* ---- identity states per pair of individuals: Jacquard's nine, IBD0 / IBD1 / IBD2 and fraternity without a dump (csrc/gev_identity.h) --
 * The per-pair reading of the interval lists at the level of individuals.  f_r(x) is taken as in gev_ibd_sharing: the (root_population,
 * hap_index) of the part of row r with st <= x < en, labels compared whole, undefined where nothing covers x.  New mutations play no
 * part.  For individual a_begin + i of pop_a (rows 2i, 2i+1 = a0, a1) against individual b_begin + k of pop_b (rows 2k, 2k+1 = b0, b1)
 * a position counts only where all four rows are covered.  There the equalities among the four labels are a partition of
 * {a0, a1, b0, b1}, one of 15; as restricted-growth strings in the order a0 a1 b0 b1 they are Jacquard's condensed identity states
 *   D1 0000                  all four IBD
 *   D2 0011                  each autozygous, different founders
 *   D3 0001 0010             a autozygous, shared with one haplotype of b
 *   D4 0012                  a autozygous, b's two distinct, nothing shared
 *   D5 0100 0111             b autozygous, shared with one haplotype of a
 *   D6 0122                  b autozygous, nothing shared
 *   D7 0101 0110             both of a's haplotypes IBD with b's, pairwise
 *   D8 0102 0120 0112 0121   exactly one pair across
 *   D9 0123                  nothing shared
 * bp[s][i][k] (uint64, plane-major [9][n_a][n_b], plane s - 1 for Ds) = the base pairs of the chromosome in state Ds.  Plain 64-bit
 * integers: exact and the same bytes on every run.  The nine planes sum to the length along which all four rows are covered.  The
 * ranges may overlap, coincide or lie in different populations; an individual against itself is D1 where it is autozygous and D7
 * elsewhere; swapping the sides swaps D3 with D5 and D4 with D6.  Kinship is (4 D1 + 2 (D3 + D5 + D7) + D8) / (4 sum), IBD2 = D1 + D7,
 * IBD1 = D3 + D5 + D8, IBD0 = D2 + D4 + D6 + D9 (geneevolve_amd/identity.py).
 * a_begin, n_a, b_begin, n_b count INDIVIDUALS.  One workgroup takes a tile of 16 x 16 pairs of individuals, one pair per lane, each
 * lane walking its four lists with four cursors where they lie; nothing bounds a row's length.  Begins as gev_ibd_sharing, for both
 * populations (a pending order is materialised, the CSR lists are derived if need be), so it works after gev_migrate, after an import
 * and on contexts without genotype planes, returns its GEV_ESTATE refusals with the same messages and returns only when the results
 * are in the caller's memory.  GEV_EINVAL for a range beyond n_people and for a NULL bp with something to write; n_a == 0 or
 * n_b == 0 touches nothing.  The results leave in sub-blocks of at most 2048 individuals a side (gev_dbg_output_chunk caps them), nine
 * planes in scratch the context owns, created by the first call. */
int gev_identity_states(gev_ctx*, int chr, int pop_a, size_t a_begin, size_t n_a,
                        int pop_b, size_t b_begin, size_t n_b, uint64_t* bp /* [9][n_a][n_b] */);
/* the same walk (csrc/gev_identity.h) compiled for the host on lists in host memory as gev_download_intervals returns them, with the
 * refusals of gev_dbg_ibd_host: no device, no context.  n_a, n_b count individuals: off_* has 2 n_* + 1 entries, rows 2i and 2i+1 are
 * individual i; along a row neither st nor en decreases.  bp as above. */
int gev_dbg_identity_host(const gev_part* parts_a, const uint64_t* off_a, size_t n_a,
                          const gev_part* parts_b, const uint64_t* off_b, size_t n_b, uint64_t* bp);
/* ---- founder lineages along the genome: local ancestry and lineage counts per position, without a dump (csrc/gev_lineage.h) ---------
 * The per-position reading of the interval lists.  f_r(x) is taken as in gev_ibd_sharing: the (root_population, hap_index) of the part
 * of row r with st <= x < en, undefined where no part covers x (parts with st >= en, gaps, rows without parts, positions before the
 * first part or at or behind the last en cover nothing).  New mutations play no part.  The caller gives n_founder_haps[n_pop] (n_pop
 * of gev_create): the founder haplotypes of each root population in its own numbering; any count at or above the largest hap_index + 1
 * is legal.  base[p] is the exclusive prefix sum and F the total; the FOUNDER ID of a covered position is fid = base[root_population] +
 * hap_index (uint32), GEV_NO_FOUNDER marks an uncovered one; F > 2^32 - 2 is GEV_EUNSUPPORTED.  pos[n_pos] are arbitrary positions in
 * non-decreasing order (duplicates allowed; an unsorted array is GEV_EINVAL).  GEV_EINVAL with nothing written, raised from a device
 * flag as gev_ancestry_bp raises its own, when any part of the rows of the range -- covering a position or not -- has a
 * root_population outside [0, n_pop) or a hap_index >= n_founder_haps[root_population].
 *
 * gev_founder_at: fid[p][i] (uint32 [n_pos][n_rows], position-major) = the founder id of row row_begin + i at pos[p].
 * gev_founder_counts, per position over the rows of the range, each output may be NULL:
 *   counts[p][f]     (uint32 [n_pos][F])      the rows with founder id f
 *   site[p]          (gev_lineage_site)       n_covered = the sum of counts, n_lineages = the founders with a non-zero count, sum_sq = the
 *                                             sum of counts^2, top_count = the largest count, top_founder = the LOWEST fid that has it
 *                                             (GEV_NO_FOUNDER when n_covered == 0)
 *   pop_counts[p][q] (uint32 [n_pos][n_pop])  the rows whose covering part has root population q
 * Plain integers: exact and the same bytes on every run.  n_covered^2 / sum_sq is the founder-genome equivalents at the position and
 * (sum_sq - n) / (n (n - 1)), n = n_covered, the probability that two distinct covered rows are identical by descent there.
 * n_rows == 0 writes zeros (a zeroed site with top_founder = GEV_NO_FOUNDER) into the per-position outputs of gev_founder_counts and
 * touches nothing else; n_pos == 0 touches nothing.
 *
 * Store and sum, no adds into global memory: a label kernel (one thread per row, the lanes of a wave stepping through the sorted
 * positions together, each with its own part cursor placed by bisection) stores fid[p][row]; a second kernel, one workgroup per
 * (position, tile of gev_dbg_lineage_tile() founders), counts the position's labels in on-chip bins and reduces them; with several
 * tiles a small third kernel folds the tiles' partial records in tile order.  The positions go in batches of about 256 MB of labels
 * (gev_dbg_output_chunk caps a batch's positions); the labels, and the counts when asked for, live in scratch the context owns,
 * created by the first call.  Both calls begin as gev_ibd_sharing (a pending order is materialised, the CSR lists are derived if need
 * be), so they work after gev_migrate, after an import and on contexts without genotype planes, return its GEV_ESTATE refusals with
 * the same messages (interval tracking off, an inactive chromosome, a population without a current generation, a generation pending)
 * and return only when the results are in the caller's memory.  GEV_EINVAL for a range beyond 2 * n_people, a NULL n_founder_haps, a
 * NULL pos with n_pos > 0, a NULL fid with something to write. */
#define GEV_NO_FOUNDER 0xffffffffu
typedef struct gev_lineage_site { uint64_t sum_sq; uint32_t n_covered, n_lineages, top_count, top_founder; } gev_lineage_site; /* 24 bytes */
int gev_founder_at(gev_ctx*, int pop, int chr, size_t row_begin, size_t n_rows, const uint64_t* pos, size_t n_pos,
                   const uint64_t* n_founder_haps /*[n_pop]*/, uint32_t* fid /* [n_pos][n_rows], position-major */);
int gev_founder_counts(gev_ctx*, int pop, int chr, size_t row_begin, size_t n_rows, const uint64_t* pos, size_t n_pos,
                       const uint64_t* n_founder_haps, uint32_t* counts /*[n_pos][F]*/, gev_lineage_site* site /*[n_pos]*/,
                       uint32_t* pop_counts /*[n_pos][n_pop]*/);
/* the same walk and reductions (csrc/gev_lineage.h) compiled for the host on lists in host memory as gev_download_intervals returns them
 * (off: n_rows + 1 entries; along a row neither st nor en decreases), with the same refusals of the positions, the founder counts and
 * the labels: no device, no context.  fid as gev_founder_at's, the others as gev_founder_counts'; each may be NULL. */
int gev_dbg_lineage_host(const gev_part* parts, const uint64_t* off, size_t n_rows, const uint64_t* pos, size_t n_pos,
                         const uint64_t* n_founder_haps, int n_pop, uint32_t* fid, uint32_t* counts, gev_lineage_site* site, uint32_t* pop_counts);
unsigned gev_dbg_lineage_tile(void);   /* founder bins a workgroup histograms at once (tests place a population across that edge) */
/* ---- runs of homozygosity: F_ROH, islands and the run list without a dump (csrc/gev_roh.h) -----------------------------------------
 * The observed side of what gev_ibd_sharing gives from the ancestry: for individual i of (pop, chr) and the SNPs [snp_begin, +n_snps),
 * hom(j) is true when haplotype rows 2i and 2i+1 carry the same allele at SNP j of the current generation (new mutations applied as
 * gev_download_haps applies them: !founder at every SNP column whose position is in the row's mutation list, idempotent).  A RUN is a
 * maximal set of consecutive SNPs j0..j1 INSIDE THE RANGE with hom true throughout and, for max_gap_bp != 0, pos[j] - pos[j-1] <=
 * max_gap_bp for every j0 < j <= j1.  SNPs outside the range do not exist for the call: runs are cut at the range's ends, so results
 * are NOT additive over SNP ranges.  A run has n = j1 - j0 + 1 SNPs, st = pos[j0] and en = pos[j1], both inclusive (PLINK's POS1 and
 * POS2), and en - st base pairs (a one-SNP run has length 0); SNP columns that share a position are consecutive SNPs with gap 0.  A run
 * QUALIFIES when n >= max(min_snps, 1) and en - st >= min_bp.  No heterozygous or missing call is allowed inside a run (simulated
 * genotypes have neither): PLINK's --homozyg with --homozyg-window-het 0, without its sliding window.  Each limit: 0 = none.
 *
 * gev_roh_summary, per individual ind_begin + i over its qualifying runs, each output may be NULL:
 *   n_roh    (uint32 [n_ind])  their number                      roh_bp (uint64 [n_ind])  their summed en - st
 *   roh_snps (uint32 [n_ind])  their summed n                    max_bp (uint64 [n_ind])  the longest en - st, 0 without a run
 *   cover    (uint32 [n_snps]) entry j: the individuals of the range with SNP snp_begin + j inside a qualifying run (ROH islands)
 * n_ind == 0 writes zeros into cover and touches nothing else; n_snps == 0 writes zeros into the per-individual vectors.
 *
 * gev_roh_segments: one record per qualifying run, ind the absolute individual, snp_first = j0 the absolute SNP index, sorted by
 * (ind, snp_first): the same bytes on every run, whatever the passes were.  out, capacity and n_total follow gev_ibd_segments' rule:
 *   *n_total is always set to the number of records of the request (n_total == NULL: GEV_EINVAL).  out is filled if and only if
 *   *n_total <= capacity; otherwise the call still returns GEV_OK, the caller sees *n_total > capacity and nothing of out is written
 *   (never a byte at or beyond out[capacity]).  out == NULL with capacity == 0 is the count-only form; a call with the counted capacity
 *   then fills.  n_ind == 0 or n_snps == 0 sets *n_total = 0 and touches nothing else.  A refused call leaves both as they were.
 *
 * Both begin like the other genotype output calls (a pending order is materialised, the planes are waited for, the CSR lists derived)
 * and return when the results are in the caller's memory.  The rows are staged, mutations applied, in passes of individuals (about
 * 256 MB of rows; gev_dbg_output_chunk caps a pass's individuals): one extra write and read of the rows, because a sparse mutation can
 * split or join a run and no after-the-fact correction exists.  One wave scans one individual, 8192 SNPs a step.  gev_roh_segments on
 * a request of one pass counts, scans and fills on the same staged rows; a request of several passes counts them all, then -- when out
 * holds the records -- stages every pass again to count and fill it: twice the staging and three scans instead of two.  A pass's
 * records are held on the device until they are copied out.  GEV_ESTATE, the message naming what is missing: no resident genotype
 * planes, an inactive chromosome, a population without a current generation, a generation pending; GEV_EINVAL for a range beyond L or
 * n_people and for params == NULL.  The device buffers are created by the first call. */
typedef struct gev_roh_params  { uint32_t min_snps, reserved; uint64_t min_bp, max_gap_bp; } gev_roh_params;   /* 0 = no limit, each */
typedef struct gev_roh_segment { uint64_t st, en; uint32_t ind, snp_first, n_snps, reserved; } gev_roh_segment; /* 32 bytes; reserved = 0 */
int gev_roh_summary(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind, const gev_roh_params*,
                    uint32_t* n_roh /*[n_ind]*/, uint64_t* roh_bp /*[n_ind]*/, uint32_t* roh_snps /*[n_ind]*/, uint64_t* max_bp /*[n_ind]*/,
                    uint32_t* cover /*[n_snps]*/);
int gev_roh_segments(gev_ctx*, int pop, int chr, size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind, const gev_roh_params*,
                     gev_roh_segment* out, size_t capacity, uint64_t* n_total);
/* the same word logic (csrc/gev_roh.h) compiled for the host on haplotype-major rows as gev_download_haps returns them (row r = bits +
 * r * row_stride_words, rows 2i and 2i+1 = individual i of n_people) and the chromosome's L positions: no device, no context, the same
 * range checks.  The summary outputs as gev_roh_summary's; the list as gev_roh_segments', n_total == NULL: no list wanted. */
int gev_dbg_roh_host(const uint64_t* bits, size_t row_stride_words, size_t n_people, size_t L, const uint64_t* pos,
                     size_t snp_begin, size_t n_snps, size_t ind_begin, size_t n_ind, const gev_roh_params*,
                     uint32_t* n_roh, uint64_t* roh_bp, uint32_t* roh_snps, uint64_t* max_bp, uint32_t* cover,
                     gev_roh_segment* out, size_t capacity, uint64_t* n_total);
/* ---- mating support [SURVEY 8(f) row 2] ------------------------------------------------------
 * == CommFunc::ras_rank (src/CommFunc.cpp:152-161), the O(n^2) zero-based rank assort_mate applies to its bivariate-normal
 * template (src/Simulation.cpp:2278-2279): rank[k] = #{x[j] < x[k]} + #{j < k : x[j] == x[k]}.  Host buffers. */
int gev_rank_f64(gev_ctx*, const double* x, size_t n, unsigned long long* rank_out);
/* ---- PLINK siblings of the dense assembly (src/Simulation.cpp:1308-1416, src/format_plink.cpp:5-141), individual-major:
 *  gev_download_plink_matrix : matrix_plink_ped of ras_convert_interval_to_format_plink (:1335-1362): row = individual
 *                              ind_begin + i, bit 2*snp + hap; ceil(L/32) words per row
 *  gev_format_ped_text       : the genotype columns format_plink::write_ped_map (:42-49) / write_ped01_map (:114-121) append
 *                              to each line: L x " a b" then '\n' = 4*L + 1 bytes per individual.  al0/al1 = one allele
 *                              letter per SNP (Legend.al0/al1, plink_map.al0/al1), or both NULL for "0"/"1" (--out_plink01).
 *                              The six id columns (FID IID PID MID sex phen, :1391-1402) are host pedigree strings: the caller
 *                              writes them in front of each line. */
int gev_download_plink_matrix(gev_ctx*, int pop, int chr, size_t ind_begin, size_t n_ind, uint64_t* bits, size_t row_stride_words);
int gev_format_ped_text(gev_ctx*, int pop, int chr, size_t ind_begin, size_t n_ind, const char* al0, const char* al1, char* out, size_t out_bytes);
/* ---- K8: genotype tiles from the interval state ------------------------------------------------
 * gev_set_dense_state(ctx, 0): keep no resident genotype planes (populations whose individuals x loci matrix exceeds HBM,
 * BASELINE config 5); the per-generation work is then sampling + interval/mutation lists + CV planes + A/D.  Call before
 * gev_init_gen0; founder SNP panels are not uploaded (gev_upload_founders is refused), CV founders are.
 * gev_materialize == ras_convert_interval_to_hap_matrix (src/Simulation.cpp:1186-1230) for haplotype rows
 * [row_begin, +n_rows) and SNPs [snp_begin, +n_snps): founder_bits = the same SNP range of every founder haplotype
 * (row = founder haplotype = part::hap_index, bit j = SNP snp_begin + j); output rows as gev_download_haps, bit j = SNP
 * snp_begin + j.  Works on dense contexts too (same result as the resident planes).  gev_materialize_pops takes one
 * founder tile per ROOT population (arrays of n_pop entries; after migration a part may descend from another population's
 * founders, :1204); gev_materialize is the single-population form. */
int gev_set_dense_state(gev_ctx*, int on);
int gev_materialize(gev_ctx*, int pop, int chr, size_t row_begin, size_t n_rows, size_t snp_begin, size_t n_snps,
                    const uint64_t* founder_bits, size_t founder_stride_words, size_t n_founder_rows,
                    uint64_t* bits, size_t row_stride_words);
/* CV genotype matrix of ras_find_cv (the --debug .cvval dump, :2665-2683), FILE column order. */
int gev_download_cv(gev_ctx*, int pop, int phen, int chr, uint64_t* bits, size_t row_stride_words);
/* ancestry interval lists (the .int output, :1596-1633): hap_offsets has 2*n_people+1 entries;
 * parts of haplotype row r are out[hap_offsets[r] .. hap_offsets[r+1]).  Call with out==NULL to
 * get the total count in *n_parts. */
int gev_download_intervals(gev_ctx*, int pop, int chr, gev_part* out, uint64_t* hap_offsets,
                           size_t* n_parts);
/* mutation positions carried by each haplotype row (union of part::mutation_pos over its
 * parts), ascending per row, duplicates kept.  Same calling convention as above. */
int gev_download_mutations(gev_ctx*, int pop, int chr, uint64_t* out, uint64_t* hap_offsets,
                           size_t* n_mut);

/* ---- introspection ------------------------------------------------------------------------ */
int gev_pop_size(gev_ctx*, int pop, size_t* n_people);
/* The resident genotype rows of the current generation (founder alleles only: mutations are kept as a sparse overlay, see
 * DESIGN.md).  A row is kept as segments_per_row segments of unit_bytes bytes; segment g of haplotype slot s = 2*individual +
 * chromatid is the unit_bytes bytes at dptr + unit_of[s * segments_per_row + g] * unit_bytes (device pointers; the last segment of
 * a row is used up to the row's length).  A segment without a crossover boundary shares the parental unit, so several entries can
 * name the same unit.  Valid until the next call that changes the population. */
int gev_plane_ptr(gev_ctx*, int pop, int chr, void** dptr, size_t* unit_bytes, size_t* n_slots, const uint32_t** unit_of, uint32_t* segments_per_row);
/* Bytes the dense stitch wrote and bytes of the rows of the generations produced, summed over all gev_reproduce calls and active
 * chromosomes of the context, and the same in row segments (the last two may be NULL).  The difference: segments that contain no
 * crossover boundary -- Simulation::recombine copies the parental parts unchanged there (src/Simulation.cpp:2939-2946, :2910) --
 * name the parent's unit instead of being copied. */
int gev_stitch_totals(gev_ctx*, unsigned long long* bytes_written, unsigned long long* bytes_total, unsigned long long* segments_written, unsigned long long* segments_total);
/* Locus-split population: mark the chromosomes whose genotype / CV / list state THIS context holds (default: all).
 * Inactive chromosomes still need gev_set_rmap / gev_set_mutmap (the rand() seed chain of Simulation::reproduce,
 * src/Simulation.cpp:2447-2501, runs through every (offspring, chromosome) task), nothing else; their A/D entries come back
 * as exact zeros, so the contexts sharing one population add their per-chromosome arrays (all-reduce) and sum over
 * chromosomes in order (geneevolve_amd/distributed.py:compute_ad_locus_split).  Call before gev_init_gen0.
 * Row movement works on such a context (gev_export_rows / gev_import_rows / gev_migrate carry the active chromosomes only: both
 * ends of an exchange must hold the same chromosomes); gev_scale_ad_compute_gef needs the all-reduced totals first (gev_set_ad). */
int gev_set_chr_active(gev_ctx*, int chr, int active);
/* reserve device capacity for populations of up to max_people (avoids reallocation) */
int gev_reserve(gev_ctx*, int pop, size_t max_people);
/* HIP stream the context launches on (hipStream_t as void*), for event timing by the caller */
int gev_stream(gev_ctx*, void** stream);
/* gev_reproduce returns when the small per-generation work is done; the dense stitch of the
 * genotype planes keeps running on a second HIP stream and every later call is ordered after it
 * where it needs the planes.  gev_sync waits for all device work of the context. */
int gev_sync(gev_ctx*);
/* on == 1 (default): the stitch overlaps later work as described above; on == 0: every generation runs on one stream and
 * gev_reproduce waits for its stitch (kernel timings without interference).  Any other value: GEV_EINVAL.
 * Environment: GEV_OVERLAP=<on> sets the initial mode. */
int gev_set_overlap(gev_ctx*, int on);
/* kernel timing measured with HIP events on the library's own streams: ms[0] = sampling
 * (crossover + mutation + seed chain), ms[1] = dense stitch (genotype planes), ms[2] = sparse state
 * (the CV planes on the main stream; the unit table and the lists run beside them on streams of their own), ms[3] = sum.  _last = most recent generation
 * (implies gev_sync); _totals = cumulative sums over all generations so far (implies gev_sync). */
int gev_last_reproduce_ms(gev_ctx*, float ms[4]);
int gev_timing_totals(gev_ctx*, double ms_sum[4], unsigned long long* n_generations);
/* generations that outgrew a buffer and were enqueued again (inside gev_reproduce_end / gev_generation_end), over the context's life */
int gev_redo_count(gev_ctx*, unsigned long long* n);
/* Simulation::ras_compute_AD (src/Simulation.cpp:2624-2749) for a population split along chromosomes over several contexts
 * (gev_set_chr_active) WITHOUT a host round trip: the per-chromosome arrays of the current generation stay on the device.
 * *add_chr / *dom_chr = device pointers to [n_people][nchr][nphen] doubles (exact zeros for the chromosomes this context does not hold),
 * *n_doubles = their length; valid until the next call that changes the population.  The caller all-reduces (SUM) both arrays in place
 * across the population's group (RCCL; every entry is x + 0 + ... + 0: bit for bit) and then calls gev_ad_finish_device. */
int gev_compute_ad_device(gev_ctx*, int pop, double** add_chr, double** dom_chr, size_t* n_doubles);
/* ... behind the in-place all-reduce: Human::additive / dominance = the sum over chromosomes in order (:2729-2746), computed on the device
 * from the (reduced) per-chromosome arrays.  The totals stay in the context for gev_scale_ad_compute_gef (as after gev_set_ad) and are
 * copied out; add_chr_out / dom_chr_out receive the reduced per-chromosome arrays.  Any of the four pointers may be NULL. */
int gev_ad_finish_device(gev_ctx*, int pop, double* additive, double* dominance, double* add_chr_out, double* dom_chr_out);
/* state of the shared list pieces of one (population, chromosome) (csrc/gev_lists.h): out[0] = times the pieces were (re)built from
 * whole lists (first use, after a migration / import / upload, arena compactions), out[1] / out[2] = interval / mutation arena
 * entries in use, out[3] / out[4] = their capacities, out[5] = position ranges per row, out[6] / out[7] = entries the last
 * generation appended, out[8] = arena compactions (unnamed pieces dropped, sharing kept), out[9] = 0.  Diagnostic: nothing observable
 * depends on it (the oracle build reports zeros). */
int gev_list_stats(gev_ctx*, int pop, int chr, unsigned long long out[10]);
/* enable/disable keeping the ancestry interval state on the device (default on) */
int gev_set_track_intervals(gev_ctx*, int on);
/* dense-stitch kernel: 0 = k_stitch_segments (default: one workgroup per entry of the list of segments to write), 1 = gamete-major
 * k_stitch_rows (every output row finds its own segments and sources).  Same results; kept for parity cross-checks. */
int gev_set_stitch_mode(gev_ctx*, int mode);
/* CV-plane stitch kernel of the following generations: 0 = automatic (default: k_stitch_small8, eight lanes per offspring row, when
 * every CV plane of the launch has sub-rows of at most 32 words that are a multiple of 4 words, a row stride that is a multiple of 4
 * words and a 16-byte aligned base; k_stitch_small, a half-wave per row, otherwise), 1 = always k_stitch_small, 2 = k_stitch_small8
 * where it is legal (today the same choice as 0).  Same rows and column counts either way; kept for parity cross-checks.  Refused
 * while a generation is pending.  gev_dbg_cv_stitch_launches: launches[0] / [1] = launches of k_stitch_small / k_stitch_small8 since
 * the context was created, so that a test can assert which form it ran. */
int gev_set_cv_stitch_form(gev_ctx*, int form);
int gev_dbg_cv_stitch_launches(gev_ctx*, unsigned long long launches[2]);

/* ---- diagnostics: RNG building blocks exposed for the parity tests (no simulation state) ----
 * gev_dbg_tables / gev_dbg_threshold / gev_dbg_canonical run on the host (table and threshold
 * construction); gev_dbg_rand / gev_dbg_sim_loc_rec run the device generators:
 * glibc srand(seed);rand()xN and one Simulation::ras_sim_loc_rec call (src/Simulation.cpp:2973). */
/* gev_dbg_verify_planes: full-coverage self-check of the dense state of a population whose founder panels came from
 * gev_synth_founders: every 32-bit word of the resident genotype plane (written by the dense stitch from breakpoints) is
 * compared on the device with ras_convert_interval_to_hap_matrix (src/Simulation.cpp:1186-1230) applied to the ancestry
 * intervals (written by the interval kernel) -- two independent paths.  founder_seeds[r] = the seed the panel of ROOT
 * population r was generated with (n_pop entries: after migration a part may descend from another population's founders, on
 * another GPU).  *n_bad_words = mismatching words, *n_bad_parts = parts whose founder is unknown / out of range (both must be 0). */
int    gev_dbg_verify_planes(gev_ctx*, int pop, int chr, const uint64_t* founder_seeds, unsigned long long* n_bad_words, unsigned long long* n_bad_parts);
/* gev_dbg_prefilter_sweep: exhaustive check of the FP64 candidate prefilter of the batched sampling kernels over the engine states
 * [x_begin, x_end) (the whole state space of minstd_rand0 is 1 .. 2^31-2) and all 256 per-lane multipliers of a scan block: out[0] = states x multipliers
 * for which the prefilter's 16-bit fraction field L deviates from the exact one, F = floor(x2 * 2^16 / M), by anything but d = L - F
 * in {0, 1} (mod 2^16), the band the scan takes its margin from (must be 0: the prefilter then flags a superset of the exact
 * candidates for every threshold), out[1] / out[2] = largest d / largest -d seen (1 and 0). */
int    gev_dbg_prefilter_sweep(gev_ctx*, uint32_t x_begin, uint32_t x_end, unsigned long long out[3]);
/* gev_dbg_output_chunk: no staging pass of the following genotype output calls takes more than max_units haplotype rows / individuals /
 * SNPs (SNPs: rounded down to a multiple of 64, at least 64), so that small tests run many passes; 0 = the byte budgets again.  Refused while a generation is pending. */
int    gev_dbg_output_chunk(gev_ctx*, size_t max_units);
/* gev_dbg_bitprod_tiles: the tile size of the matrix-core products of the following gev_pair_genotype_counts / gev_ld_counts /
 * gev_ld_scores calls.  mode 0 = by the device's compute units (the default: tiles of 128 x 128 where a sub-block has at least as many
 * of them as the device has compute units, of 64 x 64 otherwise), 1 = always 64 x 64, 2 = always 128 x 128, -1 = leave the mode as it
 * is; anything else GEV_EINVAL.  launches (may be NULL): [0] / [1] = product launches on small / large tiles since the context was
 * created, so that a test can assert which instantiation it ran.  Results never depend on the mode.  Refused while a generation is pending. */
int    gev_dbg_bitprod_tiles(gev_ctx*, int mode, unsigned long long launches[2]);
/* gev_dbg_pool_stats: out[0] = times the free list of a population's segment unit pool was rebuilt (the largest count over its active
 * chromosomes), out[1] = generations enqueued again because the free list ran out, over the context's life.  Diagnostic. */
int    gev_dbg_pool_stats(gev_ctx*, int pop, unsigned long long out[2]);
int    gev_dbg_tables(void* out, size_t bytes);
int    gev_dbg_threshold(double p, uint32_t out[4] /* a_lo, a_hi, b0, b1 */);
double gev_dbg_canonical(uint32_t a, uint32_t b);
int    gev_dbg_rand(gev_ctx*, uint32_t seed, uint32_t n, int* out);
int    gev_dbg_sim_loc_rec(gev_ctx*, int pop, int chr, uint32_t seed, uint64_t* locs, uint32_t cap,
                           uint32_t* n, int next2[2]);
/* gev_dbg_sampling_path: the sampling kernel the context launched last (which of the forms above a generation really took):
 * 0 = none yet, 1 = k_sample_batched, 2 = k_mut_sample + k_rec_sample (GEV_SAMPLE_BATCHED=0), 3 = k_rec_chain_wg (no mutation map),
 * 4 = k_rec_chain (no mutation map, GEV_CHAIN_WG=0).  gev_dbg_sim_loc_rec does not change it. */
int    gev_dbg_sampling_path(gev_ctx*, int* path);
/* gev_dbg_ad_path: the A/D kernel the context launched last: 0 = none yet, 1 = k_ad_accumulate, 2 = k_ad_accumulate_rp,
 * 3 = k_ad_accumulate_tab (rows staged), 4 = k_ad_accumulate_tab (rows read directly), 5 = k_ad_accumulate_wide; + 16 when the wide
 * kernel built its terms from the column counts itself (a generation's chain: k_stitch_small, k_cv_newmut_sum, A/D; no k_cv_finish). */
int    gev_dbg_ad_path(gev_ctx*, int* path);

#ifdef __cplusplus
}
#endif
#endif /* GENEEVOLVE_AMD_H */
