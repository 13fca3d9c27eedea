// pointing_cache.cpp -- the sealed-pointing registry (pointing_cache.hpp) and its host-memory selftest.  No device code
// and no HIP call in this file: the device side is behind Backend (runtime.cpp).
#include "pointing_cache.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

namespace toast_hip {
namespace pointing_cache {

namespace {

// Entry points that write only through the pointers they declare to the registry (wrote / wrote_rows / seal) -- the calls
// of a solver iteration, the sealing calls themselves, the arena and the cache's own entry points.  Everything else that
// passes through guarded() drops every seal.
const char * const kWhitelist[] = {
    "toast_hip_build_noise_weighted_dev",
    "toast_hip_scan_map_dev",
    "toast_hip_noise_weight_dev",
    "toast_hip_cov_apply_diag_dev",
    "toast_hip_pixels_healpix_dev",
    "stokes_weights_pol_dev",
    "toast_hip_otf_pixels_healpix_dev",
    "toast_hip_otf_stokes_weights_dev",
    "toast_hip_device_malloc",
    "toast_hip_device_free",
    "toast_hip_arena_stats",
    // the memory manager: uploads and resets declare their range, a delete frees the block
    "toast_hip_accel_present",
    "toast_hip_accel_create",
    "toast_hip_accel_create_kind",
    "toast_hip_accel_reset",
    "toast_hip_accel_update_device",
    "toast_hip_accel_update_device_parts",
    "toast_hip_accel_update_host",
    "toast_hip_accel_delete",
    "toast_hip_accel_device_ptr",
    "toast_hip_accel_generation",
    // the rest of a solver iteration: reductions, offset-template sweeps, the PCG's vector and scalar kernels
    "toast_hip_pcg_dot_dev",
    "toast_hip_pcg_step_dot_dev",
    "toast_hip_pcg_precond_diag_dot_dev",
    "toast_hip_pcg_step_dev",
    "toast_hip_pcg_stage_dev",
    "toast_hip_pcg_axpby_dev",
    "toast_hip_pcg_status_dev",
    "toast_hip_comm_allreduce_dev",
    "toast_hip_comm_map_reduce_apply_dev",
    "offset_accumulate_impl",        // (behind toast_hip_offset_[clean_]accumulate_dev)
    "offset_scan_project_launch",    // (behind toast_hip_offset_scan_project[_signal]_dev)
    "toast_hip_offset_accumulate_dev",
    "toast_hip_offset_clean_accumulate_dev",
    "toast_hip_offset_scan_project_dev",
    "toast_hip_offset_scan_project_signal_dev",
    "toast_hip_template_offset_add_to_signal_multi_dev",
    "toast_hip_template_offset_add_to_signal_dev",
    "toast_hip_template_offset_project_signal_multi_dev",
    "toast_hip_template_offset_project_signal_dev",
    "toast_hip_template_offset_apply_diag_precond_dev",
    "toast_hip_offset_accumulate_packed_dev",
    "toast_hip_offset_scan_project_packed_dev",
    "toast_hip_comm_info",
    "toast_hip_comm_available",
    "toast_hip_comm_get_mode",
    "toast_hip_comm_pixel_shard",
    "toast_hip_comm_shard_of",
    "toast_hip_pcg_state_bytes",
    "toast_hip_pointing_cache_drop",
    "toast_hip_pointing_cache_enable",
    "toast_hip_pointing_cache_stats",
    "toast_hip_pointing_cache_selftest",
};

bool overlaps(const char * lo, const char * hi, const char * a, const char * b) { return lo < b && a < hi; }

}  // namespace

bool whitelisted(const char * fn) {
    if (fn == nullptr) return false;
    for (const char * w : kWhitelist) {
        if (std::strcmp(fn, w) == 0) return true;
    }
    return false;
}

void Registry::entered(const char * fn) {
    if (!any() || whitelisted(fn)) return;
    drop_all(kDropForeignCall);
}

// ---- locking discipline: mutex_ guards the bookkeeping only.  No function of the backend that can come back into the
// registry (pack through the parameter-block cache and the arena; take / give through the arena) is called with it held:
// blocks to be released are collected under the lock and given back after it (settle).
namespace {
thread_local const Registry * t_locked = nullptr;
}

struct Registry::Lock {
    explicit Lock(Registry & r) : guard(r.mutex_) { t_locked = &r; }
    ~Lock() { t_locked = nullptr; }
    std::lock_guard<std::mutex> guard;
};

bool Registry::locked_here() const { return t_locked == this; }

void Registry::settle(Parting & parting, bool wait) {
    Parting later;
    for (const auto & b : parting) {
        if (be_.give(b.first, b.second, wait)) n_blocks_.fetch_sub(1, std::memory_order_relaxed);
        else later.push_back(b);
    }
    parting.clear();
    if (!later.empty()) {
        Lock lock(*this);
        limbo_.insert(limbo_.end(), later.begin(), later.end());
    }
}

void Registry::reap(bool wait) {
    Parting again;
    {
        Lock lock(*this);
        if (limbo_.empty()) return;
        again.swap(limbo_);
    }
    settle(again, wait);
}

void Registry::drop_at(size_t i, DropReason why, Parting & parting) {
    Seal & s = seals_[i];
    if (s.packed != nullptr) {
        st_.packed_bytes -= s.packed_bytes;
        parting.emplace_back(s.packed, s.stream);
    }
    ++st_.drops[why];
    if (i + 1 != seals_.size()) seals_[i] = std::move(seals_.back());
    seals_.pop_back();
    n_seals_.store((int)seals_.size(), std::memory_order_relaxed);
}

void Registry::drop_all(DropReason why, bool wait) {
    if (!any() && !holds_blocks()) return;
    Parting parting;
    {
        Lock lock(*this);
        while (!seals_.empty()) drop_at(seals_.size() - 1, why, parting);
    }
    settle(parting, wait);
    reap(wait);
}

void Registry::wrote(const void * p, size_t bytes, DropReason why) {
    if (!any() || p == nullptr) return;
    const char * a = static_cast<const char *>(p);
    const char * b = a + bytes;
    if (bytes == 0) {
        const char * base = nullptr;
        size_t len = 0;
        if (!be_.block_of(p, &base, &len)) return;   // not arena memory: no seal can lie there
        b = base + len;
    }
    Parting parting;
    {
        Lock lock(*this);
        for (size_t i = seals_.size(); i-- > 0;) {
            if (overlaps(seals_[i].lo, seals_[i].hi, a, b)) drop_at(i, why, parting);
        }
    }
    settle(parting, false);
}

void Registry::wrote_rows(const void * base, size_t row_bytes, const int32_t * rows, int64_t n_rows, DropReason why) {
    if (!any() || base == nullptr || n_rows <= 0) return;
    int32_t lo = rows[0], hi = rows[0];
    for (int64_t i = 1; i < n_rows; ++i) {
        lo = std::min(lo, rows[i]);
        hi = std::max(hi, rows[i]);
    }
    if (lo < 0) {
        wrote(base, 0, why);
        return;
    }
    wrote(static_cast<const char *>(base) + (size_t)lo * row_bytes, ((size_t)(hi - lo) + 1) * row_bytes, why);
}

void Registry::freed(const void * p) {
    if (!any() || p == nullptr) return;
    const char * base = nullptr;
    size_t len = 0;
    if (!be_.block_of(p, &base, &len)) return;
    Parting parting;
    {
        Lock lock(*this);
        for (size_t i = seals_.size(); i-- > 0;) {
            if (seals_[i].block == base) drop_at(i, kDropFree, parting);
        }
    }
    settle(parting, false);
}

void Registry::enable(bool on) {
    enabled_.store(on, std::memory_order_relaxed);
    if (!on) drop_all(kDropExplicit);
}

Stats Registry::stats() {
    Lock lock(*this);
    Stats s = st_;
    s.live_seals = (int64_t)seals_.size();
    return s;
}

size_t Registry::evict(bool (*wanted)(const void *)) {
    if (!holds_blocks()) return 0;
    // what was dropped earlier and could not be given back then may be all the room that is needed
    reap(true);
    Parting parting;
    size_t bytes = 0;
    {
        Lock lock(*this);
        for (Seal & s : seals_) {
            if (s.packed == nullptr || (wanted != nullptr && !wanted(s.packed))) continue;
            bytes += s.packed_bytes;
            st_.packed_bytes -= s.packed_bytes;
            parting.emplace_back(s.packed, s.stream);
            s.packed = nullptr;
            s.packed_bytes = 0;
            s.calls = 0;
            ++st_.evictions;
        }
    }
    settle(parting, true);   // the allocation that asked is waiting for this room
    return bytes;
}

void Registry::seal(Kind kind, int device, void * stream, const void * base, int64_t n_samp, const int32_t * rows,
                    int64_t n_rows, const toast_hip_interval * ivl, int64_t n_view, int64_t nside, const double * cal) {
    if (base == nullptr || n_rows <= 0 || n_samp <= 0) return;   // (nothing was written)
    reap(false);   // (copies that were dropped while their readers still ran)
    const size_t row_bytes = (size_t)n_samp * (kind == kPixels ? 8 : 24);
    // FIRST: whatever was sealed over these rows is no longer what the array holds -- whether or not this call seals
    wrote_rows(base, row_bytes, rows, n_rows, kDropReseal);
    // then every reason not to seal
    if (!enabled() || !be_.may_cache(stream)) return;
    if (n_rows > kMaxSealedRows) return;   // (one grid row of the pack kernels per sealed row)
    // pixels below 2^31: 12 nside^2 - 1 for nside <= 8192
    if (kind == kPixels && (nside <= 0 || nside > 8192)) return;
    if (kind == kWeights && cal == nullptr) return;
    Seal s;
    s.kind = kind;
    s.device = device;
    s.stream = stream;
    s.base = static_cast<const char *>(base);
    s.n_samp = n_samp;
    s.nside = nside;
    std::vector<std::pair<int32_t, double>> rc((size_t)n_rows);
    for (int64_t i = 0; i < n_rows; ++i) rc[i] = {rows[i], cal != nullptr ? cal[i] : 0.0};
    std::sort(rc.begin(), rc.end(), [](const auto & a, const auto & b) { return a.first < b.first; });
    if (rc.front().first < 0) return;
    for (size_t i = 1; i < rc.size(); ++i) {
        if (rc[i].first == rc[i - 1].first) return;   // two detectors wrote one row: which one it holds is a race
    }
    for (const auto & e : rc) {
        s.rows.push_back(e.first);
        s.cal.push_back(e.second);
    }
    s.lo = s.base + (size_t)s.rows.front() * row_bytes;
    s.hi = s.base + ((size_t)s.rows.back() + 1) * row_bytes;
    // memory the library owns, and one live block of it, or no seal
    const char * blk = nullptr;
    size_t len = 0;
    if (!be_.block_of(s.lo, &blk, &len)) return;
    if (s.hi > blk + len) return;
    s.block = blk;
    for (int64_t v = 0; v < n_view; ++v) {
        s.ivl.push_back(ivl[v].first);
        s.ivl.push_back(ivl[v].last);
    }
    Lock lock(*this);
    s.id = ++next_id_;
    seals_.push_back(std::move(s));
    n_seals_.store((int)seals_.size(), std::memory_order_relaxed);
    ++st_.seals;
}

Registry::Seal * Registry::find(Kind kind, int device, void * stream, const void * base, int64_t n_samp) {
    for (Seal & s : seals_) {
        if (s.kind == kind && s.base == base && s.device == device && s.stream == stream && s.n_samp == n_samp) return &s;
    }
    return nullptr;
}

Registry::Seal * Registry::by_id(uint64_t id) {
    for (Seal & s : seals_) {
        if (s.id == id) return &s;
    }
    return nullptr;
}

bool Registry::consume(int device, void * stream, const void * pixels, const int32_t * pixel_index, const void * weights,
                       const int32_t * weight_index, int64_t n_det, int64_t n_samp, const toast_hip_interval * ivl,
                       int64_t n_view, Hit * out) {
    if (!any()) return false;
    if (!enabled() || !be_.may_cache(stream)) return false;
    // what one seal's pack needs, copied out so that the pack runs without the lock
    struct Job {
        uint64_t id = 0;
        const char * base = nullptr;
        std::vector<int32_t> rows;
        size_t bytes = 0;
        void * block = nullptr;
    } job[2];
    {
        Lock lock(*this);
        auto miss = [&] {
            ++st_.misses;
            return false;
        };
        Seal * sp = find(kPixels, device, stream, pixels, n_samp);
        Seal * sw = find(kWeights, device, stream, weights, n_samp);
        if (sp == nullptr || sw == nullptr) return miss();
        if ((int64_t)sp->ivl.size() != 2 * n_view || sw->ivl.size() != sp->ivl.size()) return miss();
        for (int64_t v = 0; v < n_view; ++v) {
            if (sp->ivl[2 * v] != ivl[v].first || sp->ivl[2 * v + 1] != ivl[v].last) return miss();
            if (sw->ivl[2 * v] != ivl[v].first || sw->ivl[2 * v + 1] != ivl[v].last) return miss();
        }
        out->pix_row.resize((size_t)n_det);
        out->qu_row.resize((size_t)n_det);
        out->cal.resize((size_t)n_det);
        for (int64_t d = 0; d < n_det; ++d) {
            const auto ip = std::lower_bound(sp->rows.begin(), sp->rows.end(), pixel_index[d]);
            const auto iw = std::lower_bound(sw->rows.begin(), sw->rows.end(), weight_index[d]);
            if (ip == sp->rows.end() || *ip != pixel_index[d] || iw == sw->rows.end() || *iw != weight_index[d]) return miss();
            out->pix_row[d] = (int32_t)(ip - sp->rows.begin());
            out->qu_row[d] = (int32_t)(iw - sw->rows.begin());
            out->cal[d] = sw->cal[(size_t)(iw - sw->rows.begin())];
        }
        // an eligible call
        ++sp->calls;
        ++sw->calls;
        if (sp->packed != nullptr && sw->packed != nullptr) {
            out->pix = static_cast<const int32_t *>(sp->packed);
            out->qu = static_cast<const double *>(sw->packed);
            ++st_.hits;
            return true;
        }
        if (sp->calls < kPackAfterCalls || sw->calls < kPackAfterCalls) return miss();
        if (sp->packing || sw->packing) return miss();   // (another thread is at it)
        sp->packing = sw->packing = true;
        job[0].id = sp->id;
        job[1].id = sw->id;
        if (sp->packed == nullptr) {
            job[0].base = sp->base;
            job[0].rows = sp->rows;
            job[0].bytes = sp->rows.size() * (size_t)n_samp * 4;
        }
        if (sw->packed == nullptr) {
            job[1].base = sw->base;
            job[1].rows = sw->rows;
            job[1].bytes = sw->rows.size() * (size_t)n_samp * 16;
        }
    }
    // ---- the pack, without the lock: taking the blocks and launching the kernels goes through the arena and the
    // parameter-block cache, both of which may come back here (freed, evict)
    reap(false);
    bool room = true;
    for (Job & j : job) {
        if (j.bytes == 0) continue;
        j.block = be_.take(j.bytes, stream);
        room = room && j.block != nullptr;
    }
    bool launched = false;
    if (room) {
        try {
            for (int k = 0; k < 2; ++k) {
                if (job[k].bytes != 0) {
                    be_.pack(k == 0 ? kPixels : kWeights, job[k].base, job[k].block, job[k].rows.data(), (int)job[k].rows.size(),
                             n_samp, stream);
                }
            }
            launched = true;
        } catch (...) {
            launched = false;
        }
    }
    // ---- publish, if the seals are still the ones the copies were made from
    Parting parting;
    bool hit = false;
    {
        Lock lock(*this);
        Seal * sp = by_id(job[0].id);
        Seal * sw = by_id(job[1].id);
        if (sp != nullptr) sp->packing = false;
        if (sw != nullptr) sw->packing = false;
        if (launched && sp != nullptr && sw != nullptr && (job[0].bytes == 0) == (sp->packed != nullptr) &&
            (job[1].bytes == 0) == (sw->packed != nullptr)) {
            Seal * both[2] = {sp, sw};
            for (int k = 0; k < 2; ++k) {
                if (job[k].bytes == 0) continue;
                both[k]->packed = job[k].block;
                both[k]->packed_bytes = job[k].bytes;
                st_.packed_bytes += job[k].bytes;
                n_blocks_.fetch_add(1, std::memory_order_relaxed);
                job[k].block = nullptr;
            }
            out->pix = static_cast<const int32_t *>(sp->packed);
            out->qu = static_cast<const double *>(sw->packed);
            ++st_.packs;
            ++st_.hits;
            hit = true;
        } else {
            // no room in the arena's free space (the caller's arrays serve, and the next call asks again), a failed launch,
            // or a seal that was dropped meanwhile
            if (!room) ++st_.pack_no_room;
            ++st_.misses;
        }
        // blocks that were taken and are not wanted after all (counted like held ones until they are given back)
        for (Job & j : job) {
            if (j.block != nullptr) {
                n_blocks_.fetch_add(1, std::memory_order_relaxed);
                parting.emplace_back(j.block, stream);
            }
        }
    }
    settle(parting, false);
    return hit;
}

// ------------------------------------------------------------------------------------------------ selftest
namespace {

// A first-fit arena over one host buffer, with the behaviour of Manager::device_alloc that matters here: an allocation
// that finds no room evicts the packed copies and tries again.
struct HostArena {
    std::vector<char> mem;
    std::map<size_t, size_t> live;   // offset -> bytes
    void * take(size_t bytes) {
        bytes = (bytes + 15) / 16 * 16;
        size_t at = 0;
        for (const auto & b : live) {
            if (b.first - at >= bytes) break;
            at = b.first + b.second;
        }
        if (at + bytes > mem.size()) return nullptr;
        live[at] = bytes;
        return mem.data() + at;
    }
    bool give(void * p) { return live.erase((size_t)(static_cast<char *>(p) - mem.data())) == 1; }
    bool block_of(const void * p, const char ** base, size_t * bytes) const {
        const char * c = static_cast<const char *>(p);
        if (c < mem.data() || c >= mem.data() + mem.size()) return false;
        auto it = live.upper_bound((size_t)(c - mem.data()));
        if (it == live.begin()) return false;
        --it;
        if ((size_t)(c - mem.data()) >= it->first + it->second) return false;
        *base = mem.data() + it->first;
        *bytes = it->second;
        return true;
    }
};

std::mutex g_selftest_mutex;     // one selftest at a time: the backend's functions are plain pointers
HostArena * g_arena = nullptr;
bool g_may_cache = true;
bool g_lazy_give = false;        // give(wait = false) says "not yet" the first time it is asked for a block
std::vector<void *> g_asked;     // ... the blocks it was asked for once
// Every backend function reports here.  The device backend's pack goes through the parameter-block cache and the arena and
// can come back into the registry (freed, evict), and so can take and give: the stand-in does exactly that from pack --
// an allocation under pressure and a release through the harness -- and none of them may find the registry's lock held
// by the calling thread.
void backend_called(bool from_pack);

const Backend & host_backend() {
    static const Backend be = {
        [](const void * p, const char ** base, size_t * bytes) { return g_arena->block_of(p, base, bytes); },
        [](size_t bytes, void *) {
            backend_called(false);
            return g_arena->take(bytes);
        },
        [](void * p, void *, bool wait) {
            backend_called(false);
            if (g_lazy_give && !wait) {
                auto it = std::find(g_asked.begin(), g_asked.end(), p);
                if (it == g_asked.end()) {
                    g_asked.push_back(p);
                    return false;
                }
                g_asked.erase(it);
            }
            return g_arena->give(p);
        },
        [](int kind, const void * src, void * dst, const int32_t * rows, int n_rows, int64_t n_samp, void *) {
            backend_called(true);
            for (int k = 0; k < n_rows; ++k) {
                for (int64_t i = 0; i < n_samp; ++i) {
                    if (kind == kPixels) {
                        static_cast<int32_t *>(dst)[k * n_samp + i] =
                            (int32_t) static_cast<const int64_t *>(src)[(int64_t)rows[k] * n_samp + i];
                    } else {
                        const double * w = static_cast<const double *>(src) + 3 * ((int64_t)rows[k] * n_samp + i);
                        double * q = static_cast<double *>(dst) + 2 * (k * n_samp + i);
                        q[0] = w[1];
                        q[1] = w[2];
                    }
                }
            }
        },
        [](void *) { return g_may_cache; },
    };
    return be;
}

struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

// One pointing buffer pair of the model: the arrays, and what the MODEL knows about them -- independent of the
// registry's own bookkeeping: whether each array still holds what its expansion wrote.
struct ModelPair {
    int64_t * pix = nullptr;
    double * wts = nullptr;
    bool pix_clean = false, wts_clean = false;   // unchanged since the last expansion, which was allowed to seal
    int ivl_p = -1, ivl_w = -1;                  // interval list each was expanded with
    int eligible = 0;                            // consumer calls that could have hit since both were expanded
    std::vector<double> cal;
};

constexpr int kRows = 4;
constexpr int64_t kSamp = 64;

struct Harness;
Harness * g_harness = nullptr;

struct Harness {
    HostArena arena;
    Registry reg{host_backend()};
    Rng rng{1};
    std::vector<ModelPair> pairs;
    toast_hip_interval ivls[2][2];
    std::ostringstream err;
    int64_t hits = 0;
    size_t pack_pressure = 0;     // bytes that the backend's pack allocates and releases through the harness (0: none)
    int64_t pack_reentries = 0;
    bool lock_violation = false;

    void from_backend(bool from_pack) {
        if (reg.locked_here()) {
            lock_violation = true;    // (and no re-entry: it would deadlock)
            return;
        }
        if (!from_pack || pack_pressure == 0) return;
        ++pack_reentries;
        void * p = alloc(pack_pressure);
        if (p != nullptr) release(p);
    }

    explicit Harness(uint64_t seed, size_t arena_bytes) {
        rng.s = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
        arena.mem.assign(arena_bytes, 0);
        g_arena = &arena;
        g_may_cache = true;
        g_lazy_give = false;
        g_asked.clear();
        g_harness = this;
        ivls[0][0] = {0.0, 0.0, 1, 21};
        ivls[0][1] = {0.0, 0.0, 30, 61};
        ivls[1][0] = {0.0, 0.0, 1, 21};
        ivls[1][1] = {0.0, 0.0, 30, 60};
    }
    // Manager::device_alloc: evict the packed copies when there is no room, then try again
    void * alloc(size_t bytes) {
        void * p = arena.take(bytes);
        if (p == nullptr && reg.holds_blocks()) {
            reg.evict();
            p = arena.take(bytes);
        }
        return p;
    }
    void release(void * p) {
        reg.freed(p);
        arena.give(p);
    }
    bool add_pair() {
        ModelPair m;
        m.pix = static_cast<int64_t *>(alloc(kRows * kSamp * 8));
        if (m.pix == nullptr) return false;
        m.wts = static_cast<double *>(alloc(kRows * kSamp * 24));
        if (m.wts == nullptr) {
            release(m.pix);
            return false;
        }
        pairs.push_back(m);
        return true;
    }
    void expand_pixels(ModelPair & m, int iv) {
        const int32_t rows[kRows] = {2, 0, 3, 1};
        for (int64_t i = 0; i < kRows * kSamp; ++i) m.pix[i] = (rng.below(8) == 0) ? -1 : (int64_t)rng.below(1 << 20);
        reg.seal(kPixels, 0, nullptr, m.pix, kSamp, rows, kRows, ivls[iv], 2, 64, nullptr);
        m.pix_clean = g_may_cache && reg.enabled();
        m.ivl_p = iv;
        m.eligible = 0;
    }
    void expand_weights(ModelPair & m, int iv) {
        const int32_t rows[kRows] = {2, 0, 3, 1};
        m.cal.assign(kRows, 0.0);
        double cal[kRows];
        for (int k = 0; k < kRows; ++k) {
            cal[k] = 1.0 + 0.001 * rng.below(1000);
            m.cal[(size_t)rows[k]] = cal[k];
        }
        for (int k = 0; k < kRows; ++k) {
            for (int64_t i = 0; i < kSamp; ++i) {
                double * w = m.wts + 3 * (k * kSamp + i);
                w[0] = m.cal[(size_t)k];
                w[1] = rng.below(1000) * 0.001;
                w[2] = rng.below(1000) * -0.002;
            }
        }
        reg.seal(kWeights, 0, nullptr, m.wts, kSamp, rows, kRows, ivls[iv], 2, 0, cal);
        m.wts_clean = g_may_cache && reg.enabled();
        m.ivl_w = iv;
        m.eligible = 0;
    }
    // a consumer call over detectors (rows) dets with interval list iv; false = the registry broke its contract
    bool consume(ModelPair & m, int iv, const std::vector<int32_t> & dets) {
        Hit h;
        const bool hit = reg.consume(0, nullptr, m.pix, dets.data(), m.wts, dets.data(), (int64_t)dets.size(), kSamp, ivls[iv], 2, &h);
        const bool allowed = m.pix_clean && m.wts_clean && m.ivl_p == iv && m.ivl_w == iv && g_may_cache && reg.enabled();
        if (allowed) ++m.eligible;
        if (!hit) return true;
        ++hits;
        if (!allowed) {
            err << "a hit on arrays that changed since they were sealed (or with other intervals)";
            return false;
        }
        if (m.eligible < kPackAfterCalls) {
            err << "a hit on eligible call " << m.eligible << " since sealing (packing is due on call " << kPackAfterCalls << ")";
            return false;
        }
        // the packed copy holds what the arrays hold, inside the intervals
        for (size_t d = 0; d < dets.size(); ++d) {
            if (h.cal[d] != m.cal[(size_t)dets[d]]) {
                err << "wrong cal for detector " << d;
                return false;
            }
            for (int v = 0; v < 2; ++v) {
                for (int64_t i = ivls[iv][v].first; i < ivls[iv][v].last; ++i) {
                    const int64_t src = (int64_t)dets[d] * kSamp + i;
                    const double * q = h.qu + 2 * ((int64_t)h.qu_row[d] * kSamp + i);
                    if ((int64_t)h.pix[(int64_t)h.pix_row[d] * kSamp + i] != m.pix[src] || q[0] != m.wts[3 * src + 1] ||
                        q[1] != m.wts[3 * src + 2] || h.cal[d] != m.wts[3 * src]) {
                        err << "the packed copy differs from the arrays at detector " << d << " sample " << i;
                        return false;
                    }
                }
            }
        }
        return true;
    }
    void dirty_all() {
        for (ModelPair & m : pairs) m.pix_clean = m.wts_clean = false;
    }
    std::string finish() {
        while (!pairs.empty()) {
            release(pairs.back().pix);
            release(pairs.back().wts);
            pairs.pop_back();
        }
        reg.drop_all(kDropExplicit, true);
        if (err.str().empty() && lock_violation) err << "a backend function was called with the registry's lock held";
        if (err.str().empty() && reg.holds_blocks()) err << "blocks still held after everything was dropped";
        if (err.str().empty() && !arena.live.empty()) err << arena.live.size() << " blocks still live at the end (a packed copy leaked)";
        if (err.str().empty() && reg.stats().packed_bytes != 0) err << "packed_bytes not back to zero";
        g_arena = nullptr;
        g_harness = nullptr;
        return err.str();
    }
};

void backend_called(bool from_pack) {
    if (g_harness != nullptr) g_harness->from_backend(from_pack);
}

std::string random_sequence(uint64_t seed, int n_ops) {
    // room for three pairs and the packed copies of about two of them: packing, eviction and "no room" all occur
    Harness h(seed, 3 * kRows * kSamp * 32 + 2 * kRows * kSamp * 20 + 512);
    const std::vector<int32_t> all = {0, 1, 2, 3}, some = {3, 1};
    g_lazy_give = true;
    for (int op = 0; op < n_ops && h.err.str().empty() && !h.lock_violation; ++op) {
        const int what = h.rng.below(100);
        // every other pack allocates under pressure and releases, from inside the backend
        h.pack_pressure = h.rng.below(2) == 0 ? 0 : 2 * kRows * kSamp * 20;
        if (h.pairs.empty() || what < 4) {
            if (h.pairs.size() < 3) h.add_pair();
            continue;
        }
        ModelPair & m = h.pairs[(size_t)h.rng.below((int)h.pairs.size())];
        if (what < 12) {
            h.expand_pixels(m, h.rng.below(4) == 0 ? 1 : 0);
        } else if (what < 20) {
            h.expand_weights(m, h.rng.below(4) == 0 ? 1 : 0);
        } else if (what < 70) {
            if (!h.consume(m, h.rng.below(8) == 0 ? 1 : 0, h.rng.below(3) == 0 ? some : all)) break;
        } else if (what < 75) {
            // a whitelisted call writes over rows of one of the arrays (a scan_map whose det_data lies there)
            const int32_t rows[2] = {(int32_t)h.rng.below(kRows), (int32_t)h.rng.below(kRows)};
            if (h.rng.below(2) == 0) {
                h.reg.wrote_rows(m.pix, kSamp * 8, rows, 2);
                m.pix[(int64_t)rows[0] * kSamp + 5] ^= 1;
                m.pix_clean = false;
            } else {
                h.reg.wrote_rows(m.wts, kSamp * 24, rows, 2);
                m.wts[3 * ((int64_t)rows[1] * kSamp + 7) + 1] += 1.0;
                m.wts_clean = false;
            }
        } else if (what < 79) {
            // a whitelisted call writes somewhere else: nothing may be dropped for it
            const int64_t before = h.reg.stats().live_seals;
            double other[4];
            h.reg.wrote(other, sizeof(other));
            if (h.reg.stats().live_seals != before) h.err << "a write outside every seal dropped one";
        } else if (what < 83) {
            h.reg.entered("toast_hip_copy_dev");   // not whitelisted: may have written anywhere
            for (ModelPair & p : h.pairs) p.pix[5] ^= 2;
            h.dirty_all();
        } else if (what < 86) {
            h.reg.entered("toast_hip_noise_weight_dev");   // whitelisted: drops nothing by itself
        } else if (what < 90) {
            // free a pair; the next owner of the memory scribbles over it
            h.release(m.pix);
            h.release(m.wts);
            h.pairs.erase(h.pairs.begin() + (&m - h.pairs.data()));
            void * p = h.alloc(kRows * kSamp * 8);
            if (p != nullptr) {
                std::memset(p, 0x5a, kRows * kSamp * 8);
                h.release(p);
            }
        } else if (what < 95) {
            // allocation pressure: a block as large as the free space plus the packed copies
            void * p = h.alloc(2 * kRows * kSamp * 20);
            if (p != nullptr) {
                std::memset(p, 0x33, 2 * kRows * kSamp * 20);
                h.release(p);
            }
        } else if (what < 97) {
            g_may_cache = !g_may_cache;   // deterministic mode / stream capture on and off
        } else {
            h.reg.drop_all(kDropExplicit);   // toast_hip_pointing_cache_drop
            h.dirty_all();
        }
    }
    const int64_t hits = h.hits, reentries = h.pack_reentries;
    std::string e = h.finish();
    if (e.empty() && n_ops >= 2000 && hits == 0) e = "no hit in the whole sequence";
    if (e.empty() && n_ops >= 2000 && reentries == 0) e = "the backend's pack never came back into the registry";
    return e;
}

std::string scenario(int which) {
    Harness h(7, 1 << 16);
    const std::vector<int32_t> all = {0, 1, 2, 3};
    auto fail = [&](const char * m) {
        if (h.err.str().empty()) h.err << m;
    };
    h.pairs.reserve(4);
    h.add_pair();
    ModelPair & m = h.pairs[0];
    h.expand_pixels(m, 0);
    h.expand_weights(m, 0);
    auto calls = [&](int n, int iv = 0) {
        for (int i = 0; i < n; ++i) {
            if (!h.consume(m, iv, all)) return;
        }
    };
    switch (which) {
        case 1:   // the pack happens at the third call
            calls(2);
            if (h.reg.stats().packs != 0 || h.reg.stats().hits != 0) fail("packed before the third call");
            calls(1);
            if (h.reg.stats().packs != 1 || h.reg.stats().hits != 1) fail("the third call did not pack and hit");
            calls(3);
            if (h.reg.stats().packs != 1 || h.reg.stats().hits != 4) fail("later calls did not hit the one copy");
            break;
        case 2:   // a different interval list gives a miss
            calls(3);
            calls(1, 1);
            if (h.reg.stats().hits != 1 || h.reg.stats().misses != 3) fail("another interval list did not miss");
            break;
        case 3: {   // a reseal discards the copy
            calls(3);
            const size_t live = h.arena.live.size();
            h.expand_pixels(m, 0);
            if (h.arena.live.size() != live - 1 || h.reg.stats().drops[kDropReseal] != 1) fail("the reseal kept the packed pixels");
            calls(2);
            if (h.reg.stats().hits != 1) fail("a hit before the resealed pixels were packed again");
            calls(1);
            if (h.reg.stats().packs != 2 || h.reg.stats().hits != 2) fail("the resealed pixels were not packed on their third call");
            break;
        }
        case 4: {   // eviction under allocation pressure, after which the allocation succeeds
            calls(3);
            const size_t room = h.arena.mem.size() - kRows * kSamp * 32 - 16;
            void * p = h.alloc(room);
            if (p == nullptr) fail("the allocation failed although evicting the copy makes room");
            if (h.reg.stats().evictions != 2 || h.reg.stats().packed_bytes != 0) fail("the packed copies were not evicted");
            calls(1);
            if (h.reg.stats().hits != 1) fail("a hit without a packed copy");
            if (p != nullptr) h.release(p);
            break;
        }
        case 5:   // a non-whitelisted call drops every seal
            calls(3);
            h.reg.entered("toast_hip_noise_weight_dev");
            if (h.reg.stats().live_seals != 2) fail("a whitelisted call dropped seals");
            h.reg.entered("toast_hip_memset_dev");
            h.dirty_all();
            if (h.reg.stats().live_seals != 0 || h.reg.stats().drops[kDropForeignCall] != 2) fail("seals survived a non-whitelisted call");
            calls(4);
            if (h.reg.stats().hits != 1) fail("a hit after a non-whitelisted call");
            break;
        case 6: {   // an expansion that does not seal still drops what it overwrites
            const int32_t rows[kRows] = {2, 0, 3, 1};
            for (int reason = 0; reason < 4 && h.err.str().empty(); ++reason) {
                h.expand_pixels(m, 0);
                h.expand_weights(m, 0);
                calls(3);
                const Stats a = h.reg.stats();
                if (a.live_seals != 2 || a.packed_bytes != (uint64_t)kRows * kSamp * 20) fail("not packed before the expansion");
                for (int64_t i = 0; i < kRows * kSamp; ++i) m.pix[i] = 7 + reason;   // the kernel rewrites the rows ...
                m.pix_clean = false;
                if (reason == 0) {   // ... in a call of more rows than a seal may have (the rows beyond are not touched here)
                    std::vector<int32_t> many((size_t)kMaxSealedRows + 1);
                    for (size_t k = 0; k < many.size(); ++k) many[k] = (int32_t)k;
                    h.reg.seal(kPixels, 0, nullptr, m.pix, kSamp, many.data(), (int64_t)many.size(), h.ivls[0], 2, 64, nullptr);
                } else if (reason == 1) {   // ... at an Nside whose pixels do not fit 32 bits
                    h.reg.seal(kPixels, 0, nullptr, m.pix, kSamp, rows, kRows, h.ivls[0], 2, 16384, nullptr);
                } else if (reason == 2) {   // ... with two detectors of the call writing one row
                    const int32_t dup[kRows] = {2, 0, 2, 1};
                    h.reg.seal(kPixels, 0, nullptr, m.pix, kSamp, dup, kRows, h.ivls[0], 2, 64, nullptr);
                } else {   // ... while nothing may be cached
                    g_may_cache = false;
                    h.reg.seal(kPixels, 0, nullptr, m.pix, kSamp, rows, kRows, h.ivls[0], 2, 64, nullptr);
                    g_may_cache = true;
                }
                const Stats b = h.reg.stats();
                // (the pixel seal and its copy are gone; case 0's hull of 65536 rows reaches over the weights as well)
                if (b.live_seals > 1 || b.drops[kDropReseal] < a.drops[kDropReseal] + 1 ||
                    b.packed_bytes > (uint64_t)kRows * kSamp * 16 || (reason != 0 && b.live_seals != 1)) {
                    h.err << "an expansion that does not seal (case " << reason << ") left the old seal or its copy alive: seals "
                          << b.live_seals << ", reseal drops " << (b.drops[kDropReseal] - a.drops[kDropReseal]) << ", packed bytes "
                          << b.packed_bytes;
                }
                const int64_t hits = b.hits;
                calls(4);
                if (h.reg.stats().hits != hits) fail("a hit on pixels that an unsealed expansion rewrote");
            }
            break;
        }
        case 7: {   // the backend's pack comes back into the registry: an allocation that evicts, and a release
            calls(3);
            h.add_pair();
            ModelPair & m2 = h.pairs[1];
            h.expand_pixels(m2, 0);
            h.expand_weights(m2, 0);
            h.pack_pressure = h.arena.mem.size() - 2 * kRows * kSamp * 32 - kRows * kSamp * 20 - 64;   // all but the second copy
            for (int i = 0; i < 3; ++i) {
                if (!h.consume(m2, 0, all)) break;
            }
            const Stats a = h.reg.stats();
            if (h.pack_reentries != 2) fail("the pack did not come back into the registry");
            if (a.evictions != 2 || a.packs != 2 || a.hits != 2) fail("the allocation inside the pack did not evict the first pair's copies");
            h.pack_pressure = 0;
            calls(1);
            if (h.reg.stats().hits != 2) fail("a hit on an evicted copy");
            break;
        }
        default:
            fail("unknown scenario");
    }
    return h.finish();
}

}  // namespace

std::string selftest(uint64_t seed, int n_ops, int which) {
    std::lock_guard<std::mutex> lock(g_selftest_mutex);
    return which == 0 ? random_sequence(seed, n_ops) : scenario(which);
}

}  // namespace pointing_cache
}  // namespace toast_hip
