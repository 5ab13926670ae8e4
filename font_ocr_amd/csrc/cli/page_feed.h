// PageFeed — the host side of `ncc`'s pipeline in front of the devices: image headers, the batch plan, the ring of batch
// slabs the decoder threads fill ahead of the device loop, and the PNG jobs those same threads encode when they have
// nothing to decode.  focr_host.h and the standard library only: it links and runs without a device.
//
// Every function that can fail returns its message (empty: fine); the caller decides how the program ends.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "focr_host.h"

class PageFeed {
public:
    struct Batch {  // pages p0 .. p0 + n of one size; page p0 + k lives in slot k of the batch's slab, w * h bytes each
        size_t p0 = 0, n = 0, w = 0, h = 0;
    };
    struct Decoded {
        uint8_t *slab = nullptr;
        std::string err;  // the first page of the batch that could not be decoded, if any
    };

    // with_pngs: queue_pngs() will be called, so workers that run out of pages stay until close_pngs()
    PageFeed(const std::vector<std::string> &paths, size_t batch_pages, unsigned n_threads, bool with_pngs)
        : paths_(paths), batch_pages_(std::max<size_t>(1, batch_pages)),
          n_threads_((unsigned)std::min<size_t>(std::max(1u, n_threads), std::max<size_t>(1, paths.size()))), pages_(paths.size()),
          png_open_(with_pngs) {}
    ~PageFeed() {
        stop();
        for (uint8_t *p : slabs_) free(p);
    }

    // Reads every header on the threads and fixes the plan: consecutive pages of one size, at most batch_pages per batch.
    std::string plan() {
        const size_t N = pages_.size();
        {
            std::atomic<size_t> next{0};
            std::vector<std::thread> th;
            for (unsigned t = 0; t < n_threads_; t++)
                th.emplace_back([&]() {
                    for (size_t i; (i = next.fetch_add(1)) < N;) {
                        char e[256] = {0};
                        if (focr_image_probe(paths_[i].c_str(), &pages_[i].w, &pages_[i].h, e, sizeof e) != 0) pages_[i].err = e[0] ? e : "?";
                    }
                });
            for (auto &t : th) t.join();
        }
        for (const Page &p : pages_)
            if (!p.err.empty()) return p.err;
        for (size_t i = 0; i < N; i++) {
            if (batches_.empty() || batches_.back().n == batch_pages_ || batches_.back().w != pages_[i].w || batches_.back().h != pages_[i].h)
                batches_.push_back(Batch{i, 0, pages_[i].w, pages_[i].h});
            pages_[i].batch = batches_.size() - 1;
            pages_[i].slot = batches_.back().n++;
            max_bytes_ = std::max(max_bytes_, batches_.back().n * pages_[i].w * pages_[i].h);
        }
        left_.resize(batches_.size());
        for (size_t b = 0; b < batches_.size(); b++) left_[b] = batches_[b].n;
        return "";
    }
    size_t n_batches() const { return batches_.size(); }
    const Batch &batch(size_t b) const { return batches_[b]; }
    size_t slab_bytes() const { return (max_bytes_ + 4095) / 4096 * 4096; }  // the largest batch, in whole memory pages

    // Starts the workers on `first` slabs of plain page-aligned memory: decoding runs while the HIP runtime comes up.
    std::string start(size_t first) {
        if (std::string e = grow(first); !e.empty()) return e;
        for (unsigned t = 0; t < n_threads_; t++) pool_.emplace_back([this] { work(); });
        return "";
    }

    // Grows the ring to `want` slabs.  The slab of batch b is slabs[b % size], so growing re-maps batch -> slab: it may
    // only happen while every batch that was given a slab lies below the old size (b % old == b == b % want), that is,
    // before batches started beyond the first lap of the ring.  Refused otherwise.
    std::string grow(size_t want) {
        want = std::min(want, n_batches());
        {
            std::lock_guard<std::mutex> lk(mu_);  // held over the allocations: address space only, nothing is touched
            if (want > slabs_.size() && started_ > slabs_.size())
                return "slab ring: cannot grow from " + std::to_string(slabs_.size()) + " slabs after " + std::to_string(started_) + " batches were started";
            while (slabs_.size() < want) {
                void *p = nullptr;
                if (posix_memalign(&p, 4096, slab_bytes()) != 0) return "out of memory";
                slabs_.push_back((uint8_t *)p);
            }
        }
        cv_.notify_all();
        return "";
    }
    // The ring, for focr_host_register (a slab that cannot be page-locked still works).  Not while grow() may run.  The
    // destructor frees the slabs: a caller that registered them unregisters them before the feed goes, or never lets it go.
    const std::vector<uint8_t *> &slabs() const { return slabs_; }

    // Blocks until every page of batch b is decoded (or failed).
    Decoded wait_decoded(size_t b) {
        Decoded d;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return left_[b] == 0; });
            d.slab = slabs_[b % slabs_.size()];
        }
        for (size_t i = batches_[b].p0; i < batches_[b].p0 + batches_[b].n && d.err.empty(); i++) d.err = pages_[i].err;
        return d;
    }
    // Batch b's slab may be refilled.  Batches retire in order.
    void retired(size_t b) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            retired_ = b + 1;
        }
        cv_.notify_all();
    }

    // Blocks while more than `limit` PNGs are queued or being written; returns the first file that could not be written.
    std::string png_throttle(size_t limit) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return png_pending_ <= limit || !png_failed_.empty(); });
        return png_failed_;
    }
    // One RGB image of w x h per path, tightly packed in *rgb, which lives until the last of them is written.
    void queue_pngs(const std::vector<std::string> &paths, std::shared_ptr<std::vector<uint8_t>> rgb, size_t w, size_t h) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t k = 0; k < paths.size(); k++) png_jobs_.push_back(PngJob{paths[k], rgb, k * w * h * 3, w, h});
            png_pending_ += paths.size();
        }
        cv_.notify_all();
    }
    // No more PNGs will come: blocks until every queued one is on disk; returns the first file that could not be written.
    std::string close_pngs() {
        std::unique_lock<std::mutex> lk(mu_);
        png_open_ = false;
        cv_.notify_all();
        cv_.wait(lk, [&] { return png_pending_ == 0; });
        return png_failed_;
    }

    void stop() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : pool_) t.join();
        pool_.clear();
    }

private:
    struct Page {
        size_t w = 0, h = 0, batch = 0, slot = 0;
        std::string err;
    };
    struct PngJob {
        std::string path;
        std::shared_ptr<std::vector<uint8_t>> rgb;  // the batch's images
        size_t off = 0, w = 0, h = 0;
    };

    void run_png_job(std::unique_lock<std::mutex> &lk) {  // mu_ held, a job queued
        PngJob j = std::move(png_jobs_.front());
        png_jobs_.pop_front();
        lk.unlock();
        const bool ok = focr_image_save_png(j.path.c_str(), j.rgb->data() + j.off, j.w, j.h, 3) == 0;
        j.rgb.reset();
        lk.lock();
        if (!ok && png_failed_.empty()) png_failed_ = j.path;
        png_pending_--;
        cv_.notify_all();
    }
    // A worker decodes, in index order, straight into its page's slot when that batch has a slab; otherwise it encodes a
    // queued PNG; once nothing is left to decode it encodes until the queue is closed.
    void work() {
        for (size_t i; (i = next_.fetch_add(1)) < pages_.size();) {
            const size_t b = pages_[i].batch;
            uint8_t *slab;
            {
                std::unique_lock<std::mutex> lk(mu_);
                for (;;) {
                    cv_.wait(lk, [&] { return stop_ || !png_jobs_.empty() || b < retired_ + slabs_.size(); });
                    if (stop_) return;
                    if (b < retired_ + slabs_.size()) break;  // decoding feeds the devices: it goes first
                    run_png_job(lk);
                }
                slab = slabs_[b % slabs_.size()];
                started_ = std::max(started_, b + 1);
            }
            const size_t bytes = batches_[b].w * batches_[b].h;
            size_t w = 0, h = 0;
            char e[256] = {0};
            if (focr_image_load_luma8_into(paths_[i].c_str(), slab + pages_[i].slot * bytes, bytes, &w, &h, e, sizeof e) != 0)
                pages_[i].err = e[0] ? e : "?";
            else if (w != pages_[i].w || h != pages_[i].h)
                pages_[i].err = paths_[i] + ": size changed between header and decode";
            std::lock_guard<std::mutex> lk(mu_);
            if (--left_[b] == 0) cv_.notify_all();
        }
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || !png_jobs_.empty() || !png_open_; });
            if (stop_ || png_jobs_.empty()) return;  // stopped, or closed and drained
            run_png_job(lk);
        }
    }

    const std::vector<std::string> &paths_;
    const size_t batch_pages_;
    const unsigned n_threads_;
    std::vector<Page> pages_;      // w, h, batch, slot: fixed by plan(); err: written by the page's worker before left_ drops
    std::vector<Batch> batches_;
    size_t max_bytes_ = 0;
    std::vector<std::thread> pool_;
    std::atomic<size_t> next_{0};  // the next page to decode

    std::mutex mu_;  // guards everything below
    std::condition_variable cv_;
    std::vector<uint8_t *> slabs_;  // slab of batch b = slabs_[b % size] once batch b - size is retired
    std::vector<size_t> left_;      // pages of batch b still to decode
    size_t retired_ = 0;            // batches whose slabs may be refilled
    size_t started_ = 0;            // batches below this were given their slab
    bool stop_ = false;
    std::deque<PngJob> png_jobs_;
    size_t png_pending_ = 0;  // queued or being written
    bool png_open_;           // more jobs may come
    std::string png_failed_;  // the first file that could not be written
};
