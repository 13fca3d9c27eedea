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

Registry::PairCopy * Registry::pair_of(uint64_t pix_id, uint64_t wts_id) {
    for (PairCopy & pc : pair_copies_) {
        if (pc.pix_id == pix_id && pc.wts_id == wts_id) return &pc;
    }
    return nullptr;
}

// a pair copy goes with EITHER of its two seals; the seal that stays counts its calls from zero, as after an eviction
void Registry::release_pair_copy(size_t k, Parting & parting) {
    PairCopy & pc = pair_copies_[k];
    if (Seal * sp = by_id(pc.pix_id)) sp->calls = 0;
    if (Seal * sw = by_id(pc.wts_id)) sw->calls = 0;
    st_.packed_bytes -= pc.bytes;
    parting.emplace_back(pc.block, pc.stream);
    if (k + 1 != pair_copies_.size()) pair_copies_[k] = std::move(pair_copies_.back());
    pair_copies_.pop_back();
}

void Registry::drop_pair_copies_of(uint64_t seal_id, Parting & parting) {
    for (size_t k = pair_copies_.size(); k-- > 0;) {
        if (pair_copies_[k].pix_id == seal_id || pair_copies_[k].wts_id == seal_id) release_pair_copy(k, parting);
    }
}

void Registry::drop_at(size_t i, DropReason why, Parting & parting) {
    Seal & s = seals_[i];
    drop_pair_copies_of(s.id, parting);
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
    for (const PairCopy & pc : pair_copies_) s.pair_escapes += pc.escapes;
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
        for (size_t k = pair_copies_.size(); k-- > 0;) {
            PairCopy & pc = pair_copies_[k];
            if (wanted != nullptr && !wanted(pc.block)) continue;
            bytes += pc.bytes;
            ++st_.evictions;
            release_pair_copy(k, parting);   // (both seals stay and count from zero)
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
    // ... and what the pair form needs: the call's detectors in twos, the interval list, the arrays
    std::vector<int32_t> pair_rows;
    std::vector<int64_t> view;
    bool try_pair = false;
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
        if (const PairCopy * pc = pair_of(sp->id, sw->id)) {
            // the pair form is all there is of these two seals: a call that does not take its detectors in the recorded
            // pairs computes from the caller's arrays
            if (!pair_hit(*pc, pixel_index, weight_index, n_det, out)) return miss();
            ++st_.hits;
            return true;
        }
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
        // The pair form is all or nothing: tried when neither array has a copy yet, the call has a pair to offer and names
        // no row twice.  Its pairs are detectors (2 b, 2 b + 1) of THIS call; a lone last detector is a pair without a B.
        try_pair = be_.pack_pairs != nullptr && n_det >= 2 && sp->packed == nullptr && sw->packed == nullptr && n_view > 0;
        if (try_pair) {
            std::vector<int32_t> seen_p(pixel_index, pixel_index + n_det), seen_w(weight_index, weight_index + n_det);
            std::sort(seen_p.begin(), seen_p.end());
            std::sort(seen_w.begin(), seen_w.end());
            try_pair = std::adjacent_find(seen_p.begin(), seen_p.end()) == seen_p.end() &&
                       std::adjacent_find(seen_w.begin(), seen_w.end()) == seen_w.end();
        }
        if (try_pair) {
            for (int64_t d = 0; d < n_det; d += 2) {
                const bool lone = d + 1 >= n_det;
                pair_rows.push_back(pixel_index[d]);
                pair_rows.push_back(lone ? -1 : pixel_index[d + 1]);
                pair_rows.push_back(weight_index[d]);
                pair_rows.push_back(lone ? -1 : weight_index[d + 1]);
            }
            view = sp->ivl;
        }
    }
    // ---- the pack, without the lock: taking the blocks and launching the kernels goes through the arena and the
    // parameter-block cache, both of which may come back here (freed, evict)
    reap(false);
    // -- the pair form first.  A probe over the head of the first interval keeps a focal plane without co-pointing pairs
    // (or with pairs of different calibration) from paying a wasted sweep; then the sweep itself, whose escape count --
    // read back from the device, which blocks on the stream once per sealing -- decides.  More than one pair-sample in a
    // hundred escaped: the block goes back and the plain form is packed in this same call.
    PairCopy made;
    bool demoted = false;
    if (try_pair) {
        const int64_t n_pairs = (int64_t)pair_rows.size() / 4;
        // the threshold's denominator: the pair-samples in view of EVERY row of the copy, a lone detector's included
        try {
            const int64_t p0 = view[0], p1 = std::min(view[1], view[0] + kPairProbeSamples);
            int64_t esc = p1 > p0 ? be_.pack_pairs(pixels, weights, pair_rows.data(), (int)n_pairs, n_samp, view.data(),
                                                   (int)n_view, p0, p1, nullptr, stream)
                                  : 0;
            if (esc >= 0 && esc * 100 > (p1 - p0) * n_pairs) {
                demoted = true;
            } else if (esc >= 0) {
                const size_t bytes = PairLayout::bytes(n_pairs, n_samp);
                void * block = be_.take(bytes, stream);
                if (block != nullptr) {
                    int64_t in_view = 0;
                    for (int64_t v = 0; v < n_view; ++v) in_view += std::max<int64_t>(view[2 * v + 1] - view[2 * v], 0);
                    try {
                        esc = be_.pack_pairs(pixels, weights, pair_rows.data(), (int)n_pairs, n_samp, view.data(), (int)n_view, 0,
                                             n_samp, block, stream);
                    } catch (...) {
                        esc = -1;
                    }
                    if (esc >= 0 && esc * 100 <= in_view * n_pairs) {
                        made.block = block;
                        made.bytes = bytes;
                        made.stream = stream;
                        made.n_pairs = n_pairs;
                        made.n_samp = n_samp;
                        made.escapes = esc;
                    } else {
                        demoted = esc >= 0;
                        Parting back;
                        n_blocks_.fetch_add(1, std::memory_order_relaxed);
                        back.emplace_back(block, stream);
                        settle(back, false);   // (before the plain form asks for its room)
                    }
                }
            }
        } catch (...) {
        }
    }
    bool room = true;
    bool launched = false;
    if (made.block == nullptr) {
        for (Job & j : job) {
            if (j.bytes == 0) continue;
            j.block = be_.take(j.bytes, stream);
            room = room && j.block != nullptr;
        }
        if (room) {
            try {
                for (int k = 0; k < 2; ++k) {
                    if (job[k].bytes != 0) {
                        be_.pack(k == 0 ? kPixels : kWeights, job[k].base, job[k].block, job[k].rows.data(),
                                 (int)job[k].rows.size(), n_samp, stream);
                    }
                }
                launched = true;
            } catch (...) {
                launched = false;
            }
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
        const bool same = sp != nullptr && sw != nullptr && (job[0].bytes == 0) == (sp->packed != nullptr) &&
                          (job[1].bytes == 0) == (sw->packed != nullptr);
        if (made.block != nullptr && same) {
            made.pix_id = sp->id;
            made.wts_id = sw->id;
            made.rows = std::move(pair_rows);
            for (int64_t k = 0; k < made.n_pairs; ++k) made.by_pixel_a.emplace_back(made.rows[(size_t)(4 * k)], (int32_t)k);
            std::sort(made.by_pixel_a.begin(), made.by_pixel_a.end());
            st_.packed_bytes += made.bytes;
            n_blocks_.fetch_add(1, std::memory_order_relaxed);
            pair_copies_.push_back(std::move(made));
            made.block = nullptr;
            hit = pair_hit(pair_copies_.back(), pixel_index, weight_index, n_det, out);
            ++st_.packs;
            ++st_.pair_packs;
            ++st_.hits;
        } else if (made.block == nullptr && launched && same) {
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
            if (demoted) ++st_.pair_demotions;   // (the pair form was tried and the plain one TAKEN)
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
        if (made.block != nullptr) {
            n_blocks_.fetch_add(1, std::memory_order_relaxed);
            parting.emplace_back(made.block, stream);
        }
    }
    settle(parting, false);
    return hit;
}

// The hit rule of the pair form: the call's detectors, taken in twos, are recorded pairs in the same A / B orientation
// (any subset of the pairs, in any order); a lone last detector is the recorded lone.
bool Registry::pair_hit(const PairCopy & pc, const int32_t * pixel_index, const int32_t * weight_index, int64_t n_det,
                        Hit * out) const {
    out->pair_row.clear();
    for (int64_t d = 0; d < n_det; d += 2) {
        const bool lone = d + 1 >= n_det;
        const auto it = std::lower_bound(pc.by_pixel_a.begin(), pc.by_pixel_a.end(), std::make_pair(pixel_index[d], (int32_t)0));
        if (it == pc.by_pixel_a.end() || it->first != pixel_index[d]) return false;
        const int32_t * r = pc.rows.data() + 4 * (size_t)it->second;
        if (r[2] != weight_index[d]) return false;
        if (lone ? (r[1] != -1 || r[3] != -1) : (r[1] != pixel_index[d + 1] || r[3] != weight_index[d + 1])) return false;
        out->pair_row.push_back(it->second);
    }
    out->pair = true;
    out->pix = nullptr;
    out->qu = nullptr;
    out->qu_a = PairLayout::qu(pc.block, pc.n_pairs, pc.n_samp);
    out->sums = PairLayout::sums(pc.block, pc.n_pairs, pc.n_samp);
    out->word = PairLayout::word(pc.block, pc.n_pairs, pc.n_samp);
    return true;
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
bool g_pair_form = true;         // false: the stand-in's pack_pairs says "not to be had" (TOAST_HIP_PAIR=0)
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
        // the pair pack on host memory: k_pack_pairs_pp's arithmetic (kernels.hip), the count "read back" at once.  The probe
        // (dst = nullptr) reports like take / give, the sweep like pack: it comes back into the registry under pressure.
        [](const void * pixels, const void * weights, const int32_t * rows, int n_pairs, int64_t n_samp, const int64_t * ivl,
           int n_view, int64_t s_begin, int64_t s_end, void * dst, void *) -> int64_t {
            backend_called(dst != nullptr);
            if (!g_pair_form) return -1;
            const int64_t * pix = static_cast<const int64_t *>(pixels);
            const double * wts = static_cast<const double *>(weights);
            double * qu = dst ? const_cast<double *>(PairLayout::qu(dst, n_pairs, n_samp)) : nullptr;
            float * sums = dst ? const_cast<float *>(PairLayout::sums(dst, n_pairs, n_samp)) : nullptr;
            int32_t * word = dst ? const_cast<int32_t *>(PairLayout::word(dst, n_pairs, n_samp)) : nullptr;
            auto sum_or_marker = [](double a, double b) {
                const double d = a + b;
                const float f = (float)d;
                return ((double)f == d && (double)f - a == b) ? f : __builtin_nanf("");
            };
            int64_t escaped = 0;
            for (int k = 0; k < n_pairs; ++k) {
                const int32_t * r = rows + 4 * k;
                const bool lone = r[1] < 0;
                for (int64_t i = s_begin; i < s_end; ++i) {
                    const int64_t pa = pix[(int64_t)r[0] * n_samp + i];
                    const int64_t pb = lone ? pa : pix[(int64_t)r[1] * n_samp + i];
                    const double * wa = wts + 3 * ((int64_t)r[2] * n_samp + i);
                    float fq = 0.0f, fu = 0.0f;
                    if (!lone && !(pa < 0 && pb < 0)) {   // (no pixel in either: the weights are never used)
                        const double * wb = wts + 3 * ((int64_t)r[3] * n_samp + i);
                        fq = sum_or_marker(wa[1], wb[1]);
                        fu = sum_or_marker(wa[2], wb[2]);
                    }
                    const int32_t w = pa == pb ? (int32_t)pa : kPairEscape;
                    bool in_view = false;
                    for (int v = 0; v < n_view; ++v) in_view = in_view || (i >= ivl[2 * v] && i < ivl[2 * v + 1]);
                    if (in_view && (w == kPairEscape || fq != fq || fu != fu)) ++escaped;
                    if (dst != nullptr) {
                        const int64_t at = (int64_t)k * n_samp + i;
                        word[at] = w;
                        qu[2 * at] = wa[1];
                        qu[2 * at + 1] = wa[2];
                        sums[2 * at] = fq;
                        sums[2 * at + 1] = fu;
                    }
                }
            }
            return escaped;
        },
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
    std::vector<int32_t> pair_dets;              // the detector list of the call that packed the pair form (empty: none live)
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
    // what the expansions write: rows (0, 1) and (2, 3) as co-pointing pairs (same pixel, same cal, opposite Q / U), with
    // B's pixel moved away in every sample from pair_escape_from on
    bool paired = false;
    int64_t pair_escape_from = kSamp;

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
        g_pair_form = true;
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
        if (paired) {
            for (int k = 1; k < kRows; k += 2) {
                for (int64_t i = 0; i < kSamp; ++i) {
                    const int64_t a = m.pix[(k - 1) * kSamp + i];
                    m.pix[k * kSamp + i] = i < pair_escape_from ? a : a + 1;
                }
            }
        }
        m.pair_dets.clear();
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
        if (paired) {   // (rows[k] and cal[k] go together: the pair's cal is its even row's)
            for (int k = 0; k < kRows; ++k) cal[k] = m.cal[(size_t)rows[k]] = m.cal[(size_t)(rows[k] & ~1)];
        }
        for (int k = 0; k < kRows; ++k) {
            for (int64_t i = 0; i < kSamp; ++i) {
                double * w = m.wts + 3 * (k * kSamp + i);
                w[0] = m.cal[(size_t)k];
                w[1] = rng.below(1000) * 0.001;
                w[2] = rng.below(1000) * -0.002;
                if (paired && (k & 1) != 0) {
                    w[1] = -w[1 - 3 * kSamp];
                    w[2] = -w[2 - 3 * kSamp];
                }
            }
        }
        m.pair_dets.clear();
        reg.seal(kWeights, 0, nullptr, m.wts, kSamp, rows, kRows, ivls[iv], 2, 0, cal);
        m.wts_clean = g_may_cache && reg.enabled();
        m.ivl_w = iv;
        m.eligible = 0;
    }
    // a consumer call over detectors (rows) dets with interval list iv; false = the registry broke its contract
    bool consume(ModelPair & m, int iv, const std::vector<int32_t> & dets) {
        Hit h;
        const int64_t pair_packs = reg.stats().pair_packs;
        const bool hit = reg.consume(0, nullptr, m.pix, dets.data(), m.wts, dets.data(), (int64_t)dets.size(), kSamp, ivls[iv], 2, &h);
        if (reg.stats().pair_packs != pair_packs) m.pair_dets = dets;   // this call packed the pair form: its twos are the pairs
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
        if (h.pair) return pair_hit_sound(m, iv, dets, h);
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
    // A hit on the pair form.  The rule: the call's detectors in twos are pairs of the call that packed, in the same
    // orientation; a lone last detector is that call's lone.  The content: what the consumer kernels reconstruct from the
    // copy -- or read from the arrays where it says "escape" -- is what the arrays hold, inside the intervals.
    bool pair_hit_sound(const ModelPair & m, int iv, const std::vector<int32_t> & dets, const Hit & h) {
        if (h.pair_row.size() != (dets.size() + 1) / 2 || h.cal.size() != dets.size()) {
            err << "a pair hit without a row per pair";
            return false;
        }
        for (size_t d = 0; d < dets.size(); d += 2) {
            const bool lone = d + 1 >= dets.size();
            bool recorded = false;
            for (size_t r = 0; r < m.pair_dets.size() && !recorded; r += 2) {
                const bool r_lone = r + 1 >= m.pair_dets.size();
                recorded = m.pair_dets[r] == dets[d] && lone == r_lone && (lone || m.pair_dets[r + 1] == dets[d + 1]) &&
                           h.pair_row[d / 2] == (int32_t)(r / 2);
            }
            if (!recorded) {
                err << "a pair hit for detectors that are not a pair of the call that packed (position " << d << ")";
                return false;
            }
            const int64_t row = h.pair_row[d / 2];
            for (size_t e = 0; e < (lone ? 1u : 2u); ++e) {
                if (h.cal[d + e] != m.cal[(size_t)dets[d + e]]) {
                    err << "wrong cal for detector " << d + e;
                    return false;
                }
            }
            for (int v = 0; v < 2; ++v) {
                for (int64_t i = ivls[iv][v].first; i < ivls[iv][v].last; ++i) {
                    const int64_t a = (int64_t)dets[d] * kSamp + i, at = row * kSamp + i;
                    const int64_t b = lone ? a : (int64_t)dets[d + 1] * kSamp + i;
                    const int32_t w = h.word[at];
                    bool ok = w == kPairEscape ? m.pix[a] != m.pix[b] : ((int64_t)w == m.pix[a] && (int64_t)w == m.pix[b]);
                    ok = ok && h.qu_a[2 * at] == m.wts[3 * a + 1] && h.qu_a[2 * at + 1] == m.wts[3 * a + 2];
                    for (int c = 0; c < 2 && ok && !lone && !(m.pix[a] < 0 && m.pix[b] < 0); ++c) {
                        const float f = h.sums[2 * at + c];
                        ok = f != f || (double)f - h.qu_a[2 * at + c] == m.wts[3 * b + 1 + c];
                    }
                    if (!ok) {
                        err << "the pair copy does not give back the arrays at detectors " << d << ", " << d + 1 << " sample " << i;
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
    const std::vector<int32_t> all = {0, 1, 2, 3}, some = {3, 1}, swapped = {2, 3, 0, 1}, split = {1, 2}, three = {0, 1, 2};
    g_lazy_give = true;
    for (int op = 0; op < n_ops && h.err.str().empty() && !h.lock_violation; ++op) {
        const int what = h.rng.below(100);
        // three packs in four allocate under pressure and release, from inside the backend
        h.pack_pressure = h.rng.below(4) == 0 ? 0 : 2 * kRows * kSamp * 20;
        if (h.pairs.empty() || what < 4) {
            if (h.pairs.size() < 3) h.add_pair();
            continue;
        }
        ModelPair & m = h.pairs[(size_t)h.rng.below((int)h.pairs.size())];
        // two expansions in three write co-pointing pairs (the pair form needs both arrays that way), one in eight of those
        // with escapes over the threshold behind the probe's reach
        h.paired = h.rng.below(3) != 0;
        h.pair_escape_from = h.rng.below(8) == 0 ? 40 : kSamp;
        if (what < 12) {
            h.expand_pixels(m, h.rng.below(4) == 0 ? 1 : 0);
        } else if (what < 20) {
            h.expand_weights(m, h.rng.below(4) == 0 ? 1 : 0);
        } else if (what < 70) {
            const int which = h.rng.below(12);
            const std::vector<int32_t> & dets = which < 6 ? all : which < 8 ? some : which < 10 ? swapped : which < 11 ? split : three;
            if (!h.consume(m, h.rng.below(8) == 0 ? 1 : 0, dets)) break;
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
    const Stats st = h.reg.stats();
    std::string e = h.finish();
    if (e.empty() && n_ops >= 2000 && hits == 0) e = "no hit in the whole sequence";
    // (a pack every few hundred steps: a long sequence takes both forms)
    if (e.empty() && n_ops >= 20000 && st.pair_packs == 0) e = "the pair form was never taken";
    if (e.empty() && n_ops >= 20000 && st.pair_demotions == 0) e = "the pair form was never demoted";
    if (e.empty() && n_ops >= 20000 && st.packs == st.pair_packs) e = "the plain form was never taken";
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
        case 8: {   // co-pointing pairs: the pair form is chosen and hit; one escape in 102 pair-samples stays within the threshold
            h.paired = true;
            h.expand_pixels(m, 0);
            h.expand_weights(m, 0);
            m.pix[3 * kSamp + 40] += 1;   // (before the first consumer call: the model's arrays ARE what was sealed)
            calls(2);
            if (h.reg.stats().packs != 0 || h.reg.stats().hits != 0) fail("packed before the third call");
            calls(1);
            Stats a = h.reg.stats();
            if (a.packs != 1 || a.pair_packs != 1 || a.hits != 1 || a.pair_demotions != 0) fail("the third call did not take the pair form and hit");
            if (a.packed_bytes != (uint64_t)(kRows / 2) * kSamp * kPairBytes) fail("the pair copy is not 28 B per pair-sample");
            if (a.pair_escapes != 1) fail("the one escaped pair-sample was not counted");
            calls(3);
            a = h.reg.stats();
            if (a.packs != 1 || a.hits != 4) fail("later calls did not hit the one pair copy");
            // a reseal of the weights alone gives the pair copy up: it belongs to both seals
            h.expand_weights(m, 0);
            if (h.reg.stats().packed_bytes != 0 || h.reg.stats().pair_escapes != 0) fail("the pair copy outlived the weight seal");
            calls(3);
            a = h.reg.stats();
            if (a.pair_packs != 2 || a.hits != 5) fail("the pair form was not packed again on the third call after the reseal");
            // TOAST_HIP_PAIR=0: the plain form
            g_pair_form = false;
            h.expand_pixels(m, 0);
            calls(3);
            a = h.reg.stats();
            if (a.pair_packs != 2 || a.packs != 3 || a.pair_demotions != 0 || a.packed_bytes != (uint64_t)kRows * kSamp * 20) {
                fail("with the pair form switched off the plain form was not taken");
            }
            g_pair_form = true;
            break;
        }
        case 9: {   // escapes over the threshold, out of the probe's reach: demoted to the plain form in the same call
            h.paired = true;
            h.pair_escape_from = 30;   // (all of the second interval, none of the first)
            h.expand_pixels(m, 0);
            h.expand_weights(m, 0);
            calls(2);
            const size_t live = h.arena.live.size();
            calls(1);
            const Stats a = h.reg.stats();
            if (a.pair_demotions != 1 || a.pair_packs != 0) fail("the pair form was not demoted");
            if (a.packs != 1 || a.hits != 1 || a.packed_bytes != (uint64_t)kRows * kSamp * 20) fail("the plain form was not packed in the same call");
            if (h.arena.live.size() != live + 2) fail("the demoted pair block was not given back");
            calls(2);
            if (h.reg.stats().hits != 3 || h.reg.stats().packs != 1) fail("later calls did not hit the plain copy");
            break;
        }
        case 10: {   // the hit rule of the pair form
            h.paired = true;
            h.expand_pixels(m, 0);
            h.expand_weights(m, 0);
            calls(3);
            if (h.reg.stats().pair_packs != 1) fail("the pair form was not taken");
            auto one = [&](std::vector<int32_t> dets, bool want, const char * what) {
                const int64_t hits = h.reg.stats().hits, misses = h.reg.stats().misses;
                if (!h.consume(m, 0, dets)) return;
                const Stats b = h.reg.stats();
                if (b.hits != hits + (want ? 1 : 0) || b.misses != misses + (want ? 0 : 1)) fail(what);
            };
            one({1, 2}, false, "a call that splits two pairs hit");
            one({2, 3, 0, 1}, true, "the pairs in another order missed");
            one({2, 3}, true, "a subset of the pairs missed");
            one({1, 0}, false, "a pair in the other orientation hit");
            one({0, 1, 2}, false, "a lone detector that was packed as the A of a pair hit");
            if (h.reg.stats().packs != 1 || h.reg.stats().packed_bytes != (uint64_t)(kRows / 2) * kSamp * kPairBytes) {
                fail("a miss on the pair form packed something");
            }
            // ... and with a lone last detector in the call that packs
            h.expand_pixels(m, 0);
            for (int i = 0; i < 3; ++i) one({2, 3, 0}, i == 2, "the third call with a lone detector did not pack and hit");
            if (h.reg.stats().pair_packs != 2) fail("the pair form with a lone detector was not taken");
            one({0}, true, "the recorded lone missed");
            one({0, 2, 3}, false, "the recorded lone as the A of a pair hit");
            one({2, 3, 1}, false, "a lone detector that was not recorded hit");
            one({2, 3, 0}, true, "the packing call's own list missed");
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
