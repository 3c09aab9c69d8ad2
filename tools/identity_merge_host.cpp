// identity_merge_host.cpp -- the route gev_identity_states replaces, as a user would have to write it: the four-list merge of
// geneevolve_amd/csrc/gev_identity.h compiled stand-alone for one host core, over lists downloaded with gev_download_intervals.
// What tools/identity_rate.py times the device call against.
// Build:  g++ -O2 -std=c++14 -shared -fPIC tools/identity_merge_host.cpp -o tools/libidentity_merge_host.so
#include "../geneevolve_amd/csrc/gev_identity.h"

// individuals [a_begin, +n_a) against [b_begin, +n_b) of one population's lists (off: 2 n_people + 1 entries): bp [9][n_a][n_b]
extern "C" void identity_merge_host(const gev_part* parts, const uint64_t* off, size_t a_begin, size_t n_a, size_t b_begin, size_t n_b, uint64_t* bp)
{
    gev_identity_host(parts, off + 2 * a_begin, n_a, parts, off + 2 * b_begin, n_b, bp);
}
