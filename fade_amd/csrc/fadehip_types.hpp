// fadehip_types.hpp — the plain constants and structs (no device code) that the host header fadehip_host.hpp shares with
// the device headers: what fadehip_kernels.hpp sizes the context's slots by, and the two argument records of
// bgzf_inflate.hpp that more than one host unit fills.  Both device headers include it for their own use.
#pragma once
#include <stdint.h>

namespace fadehip {

constexpr int STAT_PARTS = 8;  // the stats.d counters are kept as this many partial sums (stats[8 * part + k])

constexpr int NUM_CLASSES = 10;
// Work lists: one per row class of the wave kernels plus one for queries longer than 16 * 32 = 512 bases, which
// take sw_long_kernel (a thread per alignment; rare in short-read libraries, e.g. merged pairs).
constexpr int NUM_LISTS = NUM_CLASSES + 1;

struct ScoreTab {
    uint32_t prof[8];  // prof[q class] : 8 x 4-bit entries (W + open) indexed by ref class*4
    int32_t open, ext, match, mismatch;
    uint32_t rules;    // FADEHIP_RULE_* (include/fadehip.h): the assumptions about libparasail that could not be checked
};

// ---------------------------------------------------------------- run totals kept on the device
struct PlanOut {            // in the slot's counter block, read by the host after the run
    unsigned long long cand_total;   // candidates traced by pass 2 (all classes)
    unsigned long long rerun_total;  // candidates traced again because their path left the traced steps
};

// The inflater's two argument records (bgzf_inflate.hpp): the host scans the members in one unit (fadehip_bgzf.hip) and
// fills these in three, so they are declared where all of them see them.
namespace bgzf {

struct InflateBlock {  // one per BGZF member, from the host's scan of the member headers and trailers
    uint64_t src_off;  // first byte of the member's DEFLATE stream in `comp`
    uint64_t dst_off;  // where its bytes go in `out` (running sum of ISIZE)
    uint32_t src_len;  // bytes of DEFLATE stream
    uint32_t isize;    // ISIZE of the trailer
    uint32_t crc;      // CRC32 of the trailer
    uint32_t pad;
};
static_assert(sizeof(InflateBlock) == 32, "InflateBlock layout");

struct InflateArgs {
    const uint8_t *comp;         // the members, with at least 1 KB of readable bytes behind the last one
    const InflateBlock *blocks;
    uint32_t n_blocks;
    uint8_t *out;
    const uint64_t *out_shift;   // device-side: bytes added to every dst_off (bytes carried over in front), or nullptr
    uint32_t *status;            // [n_blocks] 0 = fine, INF_E_* otherwise
    uint32_t *ticket;            // [0] ticket, [1] number of failed blocks
    int check_crc;
};

}  // namespace bgzf
}  // namespace fadehip
