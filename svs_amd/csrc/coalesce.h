// Coalescing of concurrent single-query host searches (svs_index_set_coalesce, svs_multi_set_coalesce): callers that
// are in flight together share corpus passes.  Host only; the protocol is here once, svs_index and svs_multi hold one
// instance each and give it their own batched search.
//
// The first caller to find the handle idle becomes the LEADER: it drives passes until its own query is answered, then
// hands leadership to the front of the queue (or marks the handle idle).  Everybody else queues up and sleeps until a
// pass has answered them or leadership reaches them.  A pass gathers the queued queries into one batch, searches with
// k = the largest k asked for (a top-k list's first n entries are the top-n list) and copies every waiter's share into
// the waiter's own buffers; a failed pass carries its code and text to every waiter, each of which fails again on its
// own thread (svs_internal_set_error), so svs_last_error() reads the same for all of them.
#ifndef SVS_AMD_COALESCE_H
#define SVS_AMD_COALESCE_H
#include "internal.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

namespace svs {

class Coalescer {
 public:
  std::atomic<int64_t> passes{0}, queries{0};
  std::atomic<int64_t> sizes[257] = {};   // sizes[s]: passes that carried s queries

  // One shot: the NEXT pass waits (at most 5 s) until n callers are queued; 0 cancels.
  void set_hold(int n) {
    std::lock_guard<std::mutex> lk(mu_);
    hold_ = n;
  }

  // One query of d floats, top k into out_s / out_r.  batched(queries, nq, k, out_s, out_r, &count) is the handle's
  // own batched host search; whole_tiles() says, pass by pass, whether a queue that does not fill the next kernel tile
  // size (16, 32, 64, 128) leaves its tail for the following pass.  The caller holds a reference to the handle.
  template <class Search, class Rule>
  int32_t search(const float* q, int d, int k, float* out_s, int64_t* out_r, int32_t* out_count, Search&& batched,
                 Rule&& whole_tiles) {
    Waiter me;
    me.q = q; me.k = k; me.out_s = out_s; me.out_r = out_r;
    {
      std::unique_lock<std::mutex> lk(mu_);
      pending_.push_back(&me);
      if (hold_ > 0) hold_cv_.notify_all();
      if (!busy_) { busy_ = true; me.lead = true; }
      else me.cv.wait(lk, [&] { return me.done || me.lead; });
    }
    if (me.lead) {
      // drive the device until this call's own query is answered, then hand over
      std::vector<Waiter*> batch;
      while (!me.done) {
        {
          std::unique_lock<std::mutex> lk(mu_);
          if (hold_ > 0) {   // (tests / benchmarks: a pass of a chosen size; bounded, so a miscounted test cannot hang)
            const int want = hold_;
            hold_cv_.wait_for(lk, std::chrono::seconds(5), [&] { return (int)pending_.size() >= want; });
            if (hold_ == want) hold_ = 0;   // (one shot; a hold set by another thread meanwhile stays)
          }
          size_t take = std::min<size_t>(pending_.size(), 256);
          if (whole_tiles())
            for (size_t g : {(size_t)128, (size_t)64, (size_t)32, (size_t)16})
              if (take > g && take < 2 * g) { take = g; break; }
          batch.assign(pending_.begin(), pending_.begin() + take);
          pending_.erase(pending_.begin(), pending_.begin() + take);
        }
        pass(batch, d, batched);
      }
      std::lock_guard<std::mutex> lk(mu_);
      if (!pending_.empty()) {
        pending_.front()->lead = true;   // (stays queued: its own loop takes it out)
        pending_.front()->cv.notify_one();
      } else {
        busy_ = false;
      }
    }
    if (me.rc != SVS_OK) return svs_internal_set_error(me.rc, me.err.c_str());
    if (out_count) *out_count = me.count;
    return SVS_OK;
  }

 private:
  struct Waiter {   // one queued single-query call
    const float* q;
    int k, count = 0, rc = SVS_OK;
    float* out_s;
    int64_t* out_r;
    std::string err;
    bool done = false, lead = false;
    std::condition_variable cv;
  };

  // One pass for everything that queued up while the device was busy.  The calling thread (the leader) owns it.
  template <class Search>
  void pass(std::vector<Waiter*>& batch, int d, Search& batched) {
    const int nb = (int)batch.size();
    int kmax = 0;
    for (auto* w : batch) kmax = std::max(kmax, w->k);
    int rc = SVS_OK;
    int32_t count = 0;
    std::vector<float> qs, ss;
    std::vector<int64_t> rr;
    try {
      qs.resize((size_t)nb * d);
      ss.resize((size_t)nb * kmax);
      rr.resize((size_t)nb * kmax);
    } catch (const std::bad_alloc&) {
      rc = svs_internal_set_error(SVS_ERR_NOMEM, "out of host memory for a coalesced pass");
    }
    if (rc == SVS_OK) {
      for (int i = 0; i < nb; ++i) memcpy(qs.data() + (size_t)i * d, batch[i]->q, (size_t)d * sizeof(float));
      rc = batched(qs.data(), nb, kmax, ss.data(), rr.data(), &count);
    }
    const std::string err = rc == SVS_OK ? std::string() : std::string(svs_last_error());
    passes.fetch_add(1);
    queries.fetch_add(nb);
    sizes[std::min(nb, 256)].fetch_add(1);
    std::lock_guard<std::mutex> lk(mu_);
    for (int i = 0; i < nb; ++i) {
      Waiter* w = batch[i];
      w->rc = rc;
      if (rc == SVS_OK) {
        w->count = std::min(w->k, (int)count);
        memcpy(w->out_s, ss.data() + (size_t)i * kmax, (size_t)w->count * sizeof(float));
        memcpy(w->out_r, rr.data() + (size_t)i * kmax, (size_t)w->count * sizeof(int64_t));
      } else {
        w->err = err;
      }
      w->done = true;
      if (!w->lead) w->cv.notify_one();
    }
  }

  std::mutex mu_;
  std::vector<Waiter*> pending_;   // (under mu_, like busy_ and hold_)
  bool busy_ = false;
  int hold_ = 0;
  std::condition_variable hold_cv_;
};

}  // namespace svs
#endif
