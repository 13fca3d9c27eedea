// pointing_cache.hpp -- sealed-pointing registry: reuse of a packed copy of pixels / Stokes weights across the calls of a
// solver iteration (toast_hip_build_noise_weighted_dev / toast_hip_scan_map_dev; DESIGN.md "Packed pointing cache").
//
// The library may read a packed copy instead of the caller's arrays only where it can PROVE that the arrays still hold
// what the copy was made from.  The proof is provenance: a SEAL is written when one of the library's own expansion
// kernels fills rows of an array that lies inside one live block of the library's arena, and every event that could
// change those bytes afterwards -- as far as the library can see it -- drops the seal:
//   * an entry point that is not on the whitelist of "writes only through the pointers it declares" drops every seal,
//   * a whitelisted entry point drops the seals that overlap a range it writes,
//   * freeing the arena block, a Manager upload / reset / delete over it, a new sealing call over the same rows.
// Default deny: no seal, no packed copy, no hit.  A writer the library cannot see (a foreign kernel that writes into a
// sealed arena block) is the caller's to report with toast_hip_pointing_cache_drop.
//
// Host-side bookkeeping only; everything that touches a device goes through Backend, so that the registry runs on host
// memory as well (toast_hip_pointing_cache_selftest).
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/toast_hip.h"

namespace toast_hip {
namespace pointing_cache {

// A packed copy is made on the kPackAfterCalls-th eligible consumer call since sealing: packing costs about one sweep
// over the pointing and pays back after about five calls, so a one-shot binning (one or two calls) never pays it.
constexpr int kPackAfterCalls = 3;
// one grid row of the pack kernels per sealed row: an expansion of more rows drops what it overwrites and seals nothing
constexpr int64_t kMaxSealedRows = 65535;

enum DropReason {
    kDropForeignCall = 0,   // an entry point that is not whitelisted
    kDropOverlapWrite,      // a whitelisted entry point wrote over the sealed rows
    kDropFree,              // the arena block was freed
    kDropManager,           // Manager upload / reset / delete / device change over the block
    kDropReseal,            // a new sealing call over the same rows
    kDropExplicit,          // toast_hip_pointing_cache_drop / cache switched off
    kDropReasons
};

enum Kind { kPixels = 0, kWeights = 1 };

struct Backend {
    // the live arena block that contains p; false when p lies in none (memory the library does not own)
    bool (*block_of)(const void * p, const char ** base, size_t * bytes);
    // a block from the arena's FREE space (never from the driver); nullptr when there is none
    void * (*take)(size_t bytes, void * stream);
    // give a block from take() back once the work that was queued on `stream` when this was FIRST asked for the block no
    // longer reads it.  wait = false: never blocks and never synchronises (a drop can come at any time, also while some
    // stream of the thread is being captured); false = not yet -- the registry keeps the block and asks again later.
    // wait = true (an allocation needs the room now): waits for that work.
    bool (*give)(void * p, void * stream, bool wait);
    // dst row k = packed src row rows[k] (kPixels: int64 -> int32; kWeights: (I, Q, U) -> (Q, U)), queued on `stream`
    void (*pack)(int kind, const void * src, void * dst, const int32_t * rows, int n_rows, int64_t n_samp, void * stream);
    // false: this stream must not seal, pack or hit now (deterministic mode, stream capture)
    bool (*may_cache)(void * stream);
    // The pair form (PairLayout below): row k of the copy = detectors rows[4 k .. 4 k + 3] = (pixel row A, pixel row B,
    // weight row A, weight row B; B = -1: a lone detector) of the caller's arrays, samples [s_begin, s_end).  dst =
    // nullptr: nothing is written.  Returns, READ BACK from the device (blocks on `stream`; like pack it is never called
    // with the registry's lock held), the number of pair-samples of [s_begin, s_end) inside ivl (first, last, first,
    // ...) that the pair form cannot express -- the two pixels differ, or a weight sum is not exact -- or -1 when the
    // pair form is not to be had (TOAST_HIP_PAIR=0).  May be nullptr: no pair form.  The registry calls it twice per
    // pair pack -- the probe, then the sweep -- so a packing call blocks twice.  The count is held against the
    // pair-samples in view of ALL n_pairs rows (a lone detector's row never escapes and counts): escapes x 100 <= that.
    int64_t (*pack_pairs)(const void * pixels, const void * weights, const int32_t * rows, int n_pairs, int64_t n_samp,
                          const int64_t * ivl, int n_view, int64_t s_begin, int64_t s_end, void * dst, void * stream);
};

// The pair form of the packed copy: per pair of co-pointing detectors and sample one int32 word (the common global pixel,
// -1 kept, kPairEscape where the two differ), double2 (q_a, u_a) and float2 (q_a + q_b, u_a + u_b), NaN where the sum is
// not exact -- 28 B per pair-sample in ONE block: [n_pairs][n_samp] double2, then float2, then int32.
constexpr int32_t kPairEscape = INT32_MIN;       // (no pixel: 12 nside^2 <= 2^31 - 1 ... and -1 are all there is)
constexpr size_t kPairBytes = 28;
constexpr int64_t kPairProbeSamples = 256;       // the probe in front of the pair pack: this many samples of the first interval
struct PairLayout {
    static size_t bytes(int64_t n_pairs, int64_t n_samp) { return (size_t)n_pairs * (size_t)n_samp * kPairBytes; }
    static const double * qu(const void * b, int64_t, int64_t) { return static_cast<const double *>(b); }
    static const float * sums(const void * b, int64_t n_pairs, int64_t n_samp) {
        return reinterpret_cast<const float *>(static_cast<const char *>(b) + (size_t)n_pairs * (size_t)n_samp * 16);
    }
    static const int32_t * word(const void * b, int64_t n_pairs, int64_t n_samp) {
        return reinterpret_cast<const int32_t *>(static_cast<const char *>(b) + (size_t)n_pairs * (size_t)n_samp * 24);
    }
};

struct Stats {
    int64_t seals = 0;           // seals written
    int64_t packs = 0;           // consumer calls that made a packed copy
    int64_t hits = 0;            // consumer calls served from the packed copy
    int64_t misses = 0;          // consumer calls that were not (no seal, other intervals, not yet packed, no room)
    int64_t drops[kDropReasons] = {};   // seals dropped, by reason
    int64_t evictions = 0;       // packed copies given up for an allocation
    int64_t pack_no_room = 0;    // packs that found no free arena space
    int64_t live_seals = 0;
    uint64_t packed_bytes = 0;   // bytes in packed copies now
    int64_t pair_packs = 0;      // packs that took the pair form
    int64_t pair_demotions = 0;  // packs that tried the pair form (probe or full sweep) and published the plain one
    int64_t pair_escapes = 0;    // escaped pair-samples in view of the live pair copies
};

// What a consumer launches with on a hit: packed arrays and, per detector of the call, its row in each and its cal.
struct Hit {
    const int32_t * pix = nullptr;    // [rows][n_samp] global pixel, -1 kept
    const double * qu = nullptr;      // [rows][n_samp][2]
    std::vector<int32_t> pix_row, qu_row;
    std::vector<double> cal;
    // the pair form (pix and qu stay nullptr): detectors (2 b, 2 b + 1) of the call are row pair_row[b] of the copy
    bool pair = false;
    const int32_t * word = nullptr;   // [pairs][n_samp]
    const double * qu_a = nullptr;    // [pairs][n_samp][2]
    const float * sums = nullptr;     // [pairs][n_samp][2]
    std::vector<int32_t> pair_row;
};

class Registry {
public:
    explicit Registry(const Backend & be) : be_(be) {}

    // rows [n_rows] of `base` ([*][n_samp] int64 / [*][n_samp][3] double) were just filled inside `ivl` by an expansion
    // kernel queued on `stream`.  cal: [n_rows] (weights only).  Replaces whatever was sealed over the same bytes.
    void seal(Kind kind, int device, void * stream, const void * base, int64_t n_samp, const int32_t * rows, int64_t n_rows,
              const toast_hip_interval * ivl, int64_t n_view, int64_t nside, const double * cal);
    // [p, p + bytes) is about to be written (bytes = 0: from p to the end of its arena block; nothing when p is in none)
    void wrote(const void * p, size_t bytes, DropReason why = kDropOverlapWrite);
    // rows of a [*][row_bytes] array are about to be written
    void wrote_rows(const void * base, size_t row_bytes, const int32_t * rows, int64_t n_rows,
                    DropReason why = kDropOverlapWrite);
    // the arena block that starts at / contains p is about to be released
    void freed(const void * p);
    // wait: also wait for the readers of the copies, so that every block is back in the arena on return
    void drop_all(DropReason why, bool wait = false);
    // an entry point of the library was entered through guarded(): drops every seal unless `fn` is whitelisted
    void entered(const char * fn);
    // a consumer call: true = launch the packed kernels with *out
    bool consume(int device, void * stream, const void * pixels, const int32_t * pixel_index, const void * weights,
                 const int32_t * weight_index, int64_t n_det, int64_t n_samp, const toast_hip_interval * ivl, int64_t n_view,
                 Hit * out);
    // an allocation could not be served: give up the packed copies (the seals stay and count from zero) -- those for
    // which wanted() holds (nullptr: all; the caller knows which arena failed) -- and wait until they are back; bytes
    size_t evict(bool (*wanted)(const void * block) = nullptr);
    // does the calling thread hold the registry's lock?  (selftest: a backend function must never see true)
    bool locked_here() const;
    bool any() const { return n_seals_.load(std::memory_order_relaxed) != 0; }
    bool holds_blocks() const { return n_blocks_.load(std::memory_order_relaxed) != 0; }
    void enable(bool on);
    bool enabled() const { return enabled_.load(std::memory_order_relaxed); }
    Stats stats();

private:
    struct Seal {
        Kind kind;
        int device;
        void * stream;
        const char * base;
        int64_t n_samp;
        std::vector<int32_t> rows;            // sorted, unique
        std::vector<double> cal;              // per entry of rows (weights)
        std::vector<int64_t> ivl;             // first, last, first, last, ...
        int64_t nside;
        const char * lo;                      // hull of the sealed rows
        const char * hi;
        const char * block;                   // base of the arena block
        uint64_t id = 0;                      // never reused: finds the seal again after the lock was given up
        bool packing = false;                 // a consumer call is making its copy (without the lock)
        int calls = 0;                        // eligible consumer calls since sealing
        void * packed = nullptr;
        size_t packed_bytes = 0;
    };
    // A pair copy belongs to the pixel seal and the weight seal together: dropping either gives it up.
    struct PairCopy {
        uint64_t pix_id = 0, wts_id = 0;
        void * block = nullptr;
        size_t bytes = 0;
        void * stream = nullptr;
        int64_t n_pairs = 0;
        int64_t n_samp = 0;
        int64_t escapes = 0;
        std::vector<int32_t> rows;                             // per pair in pack order: pixel A, pixel B, weight A, weight B
        std::vector<std::pair<int32_t, int32_t>> by_pixel_a;   // (pixel row A, pair), sorted
    };
    struct Lock;
    using Parting = std::vector<std::pair<void *, void *>>;   // (block, stream) to be given back
    void drop_at(size_t i, DropReason why, Parting & parting);   // mutex_ held; the blocks go to `parting`
    void settle(Parting & parting, bool wait);   // mutex_ NOT held: give back; what cannot go yet waits in limbo_
    void reap(bool wait);                        // mutex_ NOT held: try limbo_ again
    Seal * find(Kind kind, int device, void * stream, const void * base, int64_t n_samp);
    Seal * by_id(uint64_t id);
    PairCopy * pair_of(uint64_t pix_id, uint64_t wts_id);
    void release_pair_copy(size_t k, Parting & parting);             // mutex_ held; the block goes to `parting`
    void drop_pair_copies_of(uint64_t seal_id, Parting & parting);   // mutex_ held
    bool pair_hit(const PairCopy & pc, const int32_t * pixel_index, const int32_t * weight_index, int64_t n_det, Hit * out) const;

    Backend be_;
    std::mutex mutex_;
    std::vector<Seal> seals_;
    std::vector<PairCopy> pair_copies_;
    Parting limbo_;              // blocks that could not be given back yet
    uint64_t next_id_ = 0;
    Stats st_;
    std::atomic<int> n_seals_{0};
    std::atomic<int> n_blocks_{0};
    std::atomic<bool> enabled_{true};
};

// is `fn` one of the entry points that write only through the pointers they declare to the registry?
bool whitelisted(const char * fn);
// the process' registry on the device arena (runtime.cpp)
Registry & global();
// seeded random sequence of seal / consume / overlapping write / free / non-whitelisted call / allocation pressure on
// host memory against a model that knows when a hit is allowed (which = 0), or one named scenario (1: the pack happens on
// the third call, 2: another interval list misses, 3: a reseal discards the copy, 4: eviction under allocation pressure,
// 5: a non-whitelisted call drops every seal, 6: an expansion that does not seal still drops what it overwrites, 7: the
// backend's pack comes back into the registry, 8: co-pointing pairs take the pair form and hit, 9: escapes over the threshold
// demote to the plain form in the same call, 10: a call that splits a pair misses); "" when sound, else what went wrong
std::string selftest(uint64_t seed, int n_ops, int which);

}  // namespace pointing_cache
}  // namespace toast_hip
