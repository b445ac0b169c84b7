// libcessec host side: the C ABI of include/cess_ec.h over the HIP kernels in kernels.hip.
//
// Owns, per codec: the (k+m) x k encode matrix (gf256.h), the run-time coefficient programs in
// HBM (encode + one per erasure pattern in an LRU cache), the plan of the last per-segment
// reconstruct, the kernel selection (KernelOpts), a private HIP stream for uploads and a staging
// area in HBM for the host-buffer API. Multi-GPU sharding lives above this library (one codec
// per device).
//
// Lifetime of device blocks (coefficient programs, per-segment plans): a block can still be read
// by kernels enqueued on any caller stream after the host has dropped it (an evicted pattern, a
// replaced plan). Blocks come from a per-codec DevPool and are never freed in place: dropping the
// last reference retires the block, and a retired block is reused or freed only once every
// launch enqueued before the retirement has completed. Each call that launches kernels reading
// pool blocks records a mark event on its stream; a block retired after mark n waits for marks
// 1..n (host-side event queries, no device-wide synchronisation).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <list>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/cess_ec.h"
#include "fftdec_cost.h"
#include "fftdec_plan.h"
#include "flag_solve.h"
#include "read_plan.h"
#include "locate_multi_rule.h"
#include "locate_rule.h"
#include "gf256.h"
#include "hashq_where.h"
#include "host_util.h"
#include "kernels.h"

namespace {

using cec::check_launch;
using cec::KernelOpts;
using cec::Layout;
using BigMat = cec::Mat<cec::kMaxShards, cec::kMaxShards>;
using WorkMat = cec::Mat<cec::kMaxShards, 2 * cec::kMaxShards>;
using BigPlan = cec::Plan<cec::kMaxShards, cec::kMaxShards>;

thread_local std::string g_last_error;

int set_err(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

// ---- device block pool with stream-ordered retirement -------------------------------------
// Blocks come from the stream-ordered allocator on the codec's private stream and go back to it
// with hipFreeAsync: hipMalloc / hipFree would do (hipFree performs an implicit
// hipDeviceSynchronize), and destroying one codec must not wait for other codecs' work.
class DevPool {
 public:
  ~DevPool() { drain(); }
  void set_stream(hipStream_t st) { st_ = st; }

  // A block of at least `bytes` (size classes of powers of two from 4 KiB).
  int alloc(size_t bytes, void** out) {
    collect();
    const int c = cls(bytes);
    if ((size_t)c < free_.size() && !free_[c].empty()) {
      *out = free_[c].back();
      free_[c].pop_back();
      return CEC_OK;
    }
    // complete before any stream uses it (a rare host wait: freed blocks are reused)
    CEC_HIP_TRY(hipMallocAsync(out, (size_t)1 << c, st_));
    CEC_HIP_TRY(hipStreamSynchronize(st_));
    held_ += (size_t)1 << c;
    return CEC_OK;
  }
  // The last reference to a block was dropped; kernels enqueued so far may still read it.
  void retire(void* p, size_t bytes) {
    if (p) dead_.push_back({seq_, p, cls(bytes)});
  }
  // Record the completion point of the launches just enqueued on `st`.
  int mark(hipStream_t st) {
    hipEvent_t ev = nullptr;
    if (!evpool_.empty()) {
      ev = evpool_.back();
      evpool_.pop_back();
    } else {
      CEC_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    hipError_t e = hipEventRecord(ev, st);
    if (e != hipSuccess) {
      evpool_.push_back(ev);
      return set_err(CEC_EHIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
    }
    marks_.push_back({++seq_, ev});
    // bound the backlog of a producer that never synchronises
    while (marks_.size() > 1024) {
      (void)hipEventSynchronize(marks_.front().ev);
      collect();
    }
    return CEC_OK;
  }
  // Move retired blocks whose readers have completed to the free lists.
  void collect() {
    while (!marks_.empty() && hipEventQuery(marks_.front().ev) == hipSuccess) {
      done_ = marks_.front().seq;
      evpool_.push_back(marks_.front().ev);
      marks_.pop_front();
    }
    if (marks_.empty()) done_ = seq_;
    while (!dead_.empty() && dead_.front().tag <= done_) {
      const Dead& d = dead_.front();
      if ((size_t)d.c >= free_.size()) free_.resize(d.c + 1);
      free_[d.c].push_back(d.p);
      dead_.pop_front();
    }
  }
  // Wait for every mark and free every block (codec destruction).
  void drain() {
    for (auto& m : marks_) {
      (void)hipEventSynchronize(m.ev);
      evpool_.push_back(m.ev);
    }
    marks_.clear();
    done_ = seq_;
    collect();
    for (auto& fl : free_)
      for (void* p : fl) (void)hipFreeAsync(p, st_);
    if (held_) (void)hipStreamSynchronize(st_);
    free_.clear();
    held_ = 0;
    for (hipEvent_t e : evpool_) (void)hipEventDestroy(e);
    evpool_.clear();
  }
  size_t pending() const { return dead_.size(); }
  size_t held() const { return held_; }  // device bytes the pool has allocated (live + free)

 private:
  static int cls(size_t bytes) {
    int c = 12;
    while (((size_t)1 << c) < bytes) ++c;
    return c;
  }
  struct Dead {
    uint64_t tag;
    void* p;
    int c;
  };
  struct Mark {
    uint64_t seq;
    hipEvent_t ev;
  };
  std::vector<std::vector<void*>> free_;
  std::deque<Dead> dead_;  // in retirement order, so tags are non-decreasing
  std::deque<Mark> marks_;
  std::vector<hipEvent_t> evpool_;
  hipStream_t st_ = nullptr;  // the owner's private stream (allocations and frees)
  uint64_t seq_ = 0;   // marks recorded
  uint64_t done_ = 0;  // every mark <= done_ has completed
  size_t held_ = 0;
};

// Batch-sized scratch (a verify's recomputed parity, an audit's gathered chunks) is not a pool
// block: the pool rounds to powers of two and keeps blocks until the codec dies, so one verify of
// ~94 GiB would pin 128 GiB of HBM to the codec. Above this size the scratch is stream-ordered
// (hipMallocAsync / hipFreeAsync on the call's stream): exact size, returned once the stream
// passes the launches that read it, no host wait.
constexpr size_t kBigScratch = size_t(16) << 20;
struct Scratch {
  void* p = nullptr;
  size_t bytes = 0;
  bool async = false;
};

// A run-time program: chunks of up to kRtMaxOut outputs, each a device block in the layout of
// kernels.h (header, input indices, output indices, coefficients [nin][nob]).
struct RtChunk {
  uint32_t* dev = nullptr;
  size_t bytes = 0;
  int nin = 0, nout = 0, nob = 0;
};

struct Program {
  std::vector<RtChunk> chunks;
  int nout = 0;     // total outputs
  int single = -1;  // the one missing shard when exactly one output (compile-time decode)
  bool partial = false;  // rows restricted to held survivors (cec_reconstruct_partial_batch)
  // RS(32,32): the same rebuild as an FFT-domain decode plan (fftdec_plan.h), a pool block
  uint32_t* fd = nullptr;
  size_t fd_bytes = 0;
  int fd_side = 0;
  int fd_nrs = 0;  // syndrome slots of the plan (its row cost: outputs x slots)
  // and as a formal-derivative plan (fftdec_plan_d: cost independent of the erasure count)
  uint32_t* fdd = nullptr;
  size_t fdd_bytes = 0;
  uint8_t in_idx[cec::kMaxShards] = {};   // survivors read (host copy)
  uint8_t out_idx[cec::kMaxShards] = {};  // shards written (host copy)
};
using ProgPtr = std::shared_ptr<const Program>;

// Upload coefficient rows for outputs out_idx[o] (coef[o][j]) as run-time chunks. The chunk
// blocks come from `pool` and go back to it (retired) when the last ProgPtr is dropped. Uploads
// run on `upload` and are complete when this returns.
// `partial`: the rows do not rebuild a shard by themselves (cec_reconstruct_partial_batch), so
// the compile-time single-erasure kernels never stand in for the program.
// Page-locked staging for program images whose uploads stay in flight until one synchronisation
// per plan: an upload from pinned memory is a DMA enqueue, one from pageable memory is staged by
// the runtime (measured: 64 new RS(32,32) patterns per call cost ~0.9 ms of host time beyond the
// kernel with pageable images). Blocks of >= 1 MiB, kept for reuse; reset() after the sync.
// hipHostFree, like hipFree, synchronises the whole device, so destroying a codec must not free
// its arena's blocks: they go to this process-wide cache (up to kCap bytes) for the next arena.
// The cache is never destroyed (the HIP runtime may be gone by the time static destructors run).
// Blocks are reused on the device they were allocated under only.
struct PinnedCache {
  static constexpr size_t kCap = size_t(64) << 20;
  struct Block {
    uint8_t* p;
    size_t cap;
    int device;
  };
  std::mutex mu;
  std::vector<Block> blocks;
  size_t bytes = 0;
  static PinnedCache& get() {
    static PinnedCache* c = new PinnedCache;
    return *c;
  }
  // a cached block of at least `need` bytes of `device` (the smallest), or {nullptr, 0, device}
  Block take(size_t need, int device) {
    std::lock_guard<std::mutex> g(mu);
    size_t best = blocks.size();
    for (size_t i = 0; i < blocks.size(); ++i)
      if (blocks[i].device == device && blocks[i].cap >= need &&
          (best == blocks.size() || blocks[i].cap < blocks[best].cap))
        best = i;
    if (best == blocks.size()) return {nullptr, 0, device};
    const Block b = blocks[best];
    blocks.erase(blocks.begin() + best);
    bytes -= b.cap;
    return b;
  }
  void give(const Block& b) {
    {
      std::lock_guard<std::mutex> g(mu);
      if (bytes + b.cap <= kCap) {
        blocks.push_back(b);
        bytes += b.cap;
        return;
      }
    }
    (void)hipHostFree(b.p);  // past the cap: the rare device-wide synchronisation
  }
};

class PinnedArena {
 public:
  ~PinnedArena() {
    for (auto& b : blocks_) PinnedCache::get().give({b.p, b.cap, device_});
  }
  // `bytes` of zeroed page-locked memory valid until reset(), or nullptr (caller falls back)
  uint32_t* take(size_t bytes) {
    bytes = (bytes + 255) & ~size_t(255);
    for (; cur_ < blocks_.size(); ++cur_)
      if (blocks_[cur_].used + bytes <= blocks_[cur_].cap) break;
    if (cur_ == blocks_.size()) {
      Block b{nullptr, std::max(bytes, size_t(1) << 20), 0};
      if (blocks_.empty() && hipGetDevice(&device_) != hipSuccess) return nullptr;
      const PinnedCache::Block cached = PinnedCache::get().take(b.cap, device_);
      if (cached.p) {
        b.p = cached.p;
        b.cap = cached.cap;
      } else if (hipHostMalloc(reinterpret_cast<void**>(&b.p), b.cap, hipHostMallocDefault) !=
                 hipSuccess) {
        return nullptr;
      }
      blocks_.push_back(b);
    }
    Block& b = blocks_[cur_];
    uint8_t* p = b.p + b.used;
    b.used += bytes;
    std::memset(p, 0, bytes);
    return reinterpret_cast<uint32_t*>(p);
  }
  void reset() {
    for (auto& b : blocks_) b.used = 0;
    cur_ = 0;
  }
  bool busy() const { return cur_ > 0 || (!blocks_.empty() && blocks_[0].used); }

 private:
  struct Block {
    uint8_t* p;
    size_t cap, used;
  };
  std::vector<Block> blocks_;
  size_t cur_ = 0;
  int device_ = -1;  // the device current when the first block was taken (the codec's)
};

// With `keep`, the images are written into that arena and the uploads are left in flight: the
// caller synchronises `upload` once for a whole plan before launching or resetting the arena.
using HostImages = PinnedArena;
int build_program(DevPool& pool, hipStream_t upload, const uint8_t* in_idx, int nin,
                  const uint8_t* out_idx, int nout, const BigMat& coef, ProgPtr* out,
                  bool partial = false, HostImages* keep = nullptr,
                  const cec::FftDecPlan* fdp = nullptr, const cec::FftDecPlan* fddp = nullptr) {
  DevPool* pp = &pool;
  std::shared_ptr<Program> prog(new Program, [pp](Program* p) {
    for (auto& c : p->chunks) pp->retire(c.dev, c.bytes);
    pp->retire(p->fd, p->fd_bytes);
    pp->retire(p->fdd, p->fdd_bytes);
    delete p;
  });
  prog->nout = nout;
  prog->single = nout == 1 && !partial ? out_idx[0] : -1;
  prog->partial = partial;
  std::memcpy(prog->in_idx, in_idx, nin);
  std::memcpy(prog->out_idx, out_idx, nout);
  std::vector<std::vector<uint32_t>> hosts;  // images when there is no arena (or it is full)
  bool staged = keep != nullptr;
  for (int o0 = 0; o0 < nout; o0 += cec::kRtMaxOut) {
    RtChunk c;
    c.nin = nin;
    c.nout = std::min(cec::kRtMaxOut, nout - o0);
    c.nob = cec::rt_bucket(c.nout);
    const size_t words = cec::rt_chunk_bytes(nin, c.nob) / sizeof(uint32_t);
    uint32_t* h = keep ? keep->take(words * sizeof(uint32_t)) : nullptr;
    if (!h) {
      hosts.emplace_back(words, 0u);
      h = hosts.back().data();
      staged = false;  // a pageable image: synchronise before it dies
    }
    h[0] = (uint32_t)nin;
    h[1] = (uint32_t)c.nout;
    h[2] = (uint32_t)c.nob;
    for (int j = 0; j < nin; ++j) h[4 + j] = in_idx[j];
    for (int o = 0; o < c.nout; ++o) h[4 + 256 + o] = out_idx[o0 + o];
    uint32_t* hb = h + 4 + 512;
    uint32_t* mk = h + cec::kRtHeaderWords;
    for (int j = 0; j < nin; ++j) {
      int top = -1;
      for (int o = 0; o < c.nout; ++o) {
        const unsigned cf = coef.v[o0 + o][j];
        for (int b = 0; b < 8; ++b)
          if (cf >> b & 1) {
            mk[((size_t)j * 8 + b) * c.nob + o] = 0xFFFFFFFFu;
            top = std::max(top, b);
          }
      }
      hb[j] = (uint32_t)top;
    }
    if (nin <= cec::kRthMaxIn) {
      // Horner section (kernels.h): per output row, its top bit and per (bit, group) the
      // combination index of the group's inputs whose coefficient has that bit
      const size_t hoff = cec::kRtHeaderWords + (size_t)nin * 8 * c.nob;
      h[3] = (uint32_t)hoff;
      uint32_t* top = h + hoff;
      uint32_t* ix = top + 32;
      for (int o = 0; o < c.nout; ++o) {
        int t = -1;
        for (int j = 0; j < nin; ++j)
          for (int b = 0; b < 8; ++b)
            if (coef.v[o0 + o][j] >> b & 1) t = std::max(t, b);
        top[o] = (uint32_t)t;
        for (int b = 0; b < 8; ++b)
          for (int j = 0; j < nin; ++j)
            if (coef.v[o0 + o][j] >> b & 1) ix[((size_t)o * 8 + b) * 8 + j / 4] |= 1u << (j % 4);
      }
    }
    c.bytes = words * sizeof(uint32_t);
    void* d = nullptr;
    int rc = pool.alloc(c.bytes, &d);
    if (rc) return rc;  // prog's deleter retires the chunks built so far
    c.dev = static_cast<uint32_t*>(d);
    prog->chunks.push_back(c);
    CEC_HIP_TRY(hipMemcpyAsync(c.dev, h, c.bytes, hipMemcpyHostToDevice, upload));
  }
  // the FFT-domain decode plans of the same pattern
  auto upload_plan = [&](const cec::FftDecPlan& fp, uint32_t** dev, size_t* dbytes) -> int {
    const size_t bytes = fp.w.size() * sizeof(uint32_t);
    uint32_t* h = keep ? keep->take(bytes) : nullptr;
    if (!h) {
      hosts.emplace_back(fp.w);
      h = hosts.back().data();
      staged = false;
    } else {
      std::memcpy(h, fp.w.data(), bytes);
    }
    void* d = nullptr;
    int rc = pool.alloc(bytes, &d);
    if (rc) return rc;
    *dev = static_cast<uint32_t*>(d);
    *dbytes = bytes;
    CEC_HIP_TRY(hipMemcpyAsync(*dev, h, bytes, hipMemcpyHostToDevice, upload));
    return CEC_OK;
  };
  if (fdp) {
    int rc = upload_plan(*fdp, &prog->fd, &prog->fd_bytes);
    if (rc) return rc;
    prog->fd_side = fdp->side;
    prog->fd_nrs = fdp->nrslots;
  }
  if (fddp) {
    int rc = upload_plan(*fddp, &prog->fdd, &prog->fdd_bytes);
    if (rc) return rc;
  }
  // the block may be a reused one whose readers have completed; the upload must land before
  // any caller-stream launch that reads it, and pageable images die here (arena images live
  // until the caller's synchronisation)
  if (!staged) CEC_HIP_TRY(hipStreamSynchronize(upload));
  *out = std::move(prog);
  return CEC_OK;
}

// One multi-pattern run-time launch of the per-segment reconstruct path.
struct PsLaunch {
  int nob = 0, nin = 0;
  size_t off = 0, count = 0;  // into the plan's segment-list / chunk-pointer arrays
};

// Plan of one per-segment reconstruct call (cached for a repeated pattern array): either
// compile-time launches per pattern (ct: program, offset, count into list), one mixed-pattern
// RS(2,1) launch, or multi-pattern run-time launches (rt: segment list + per-segment chunk
// pointers). `progs` holds every program whose device chunks the arrays point at.
struct PsPlan {
  std::string key;
  std::vector<ProgPtr> progs;
  std::vector<std::string> keys;  // decode-cache keys of the patterns (LRU touch on reuse)
  uint32_t* list = nullptr;
  size_t list_bytes = 0;
  void* ptrs = nullptr;  // const uint32_t* [count] per run-time launch
  size_t ptrs_bytes = 0;
  std::vector<std::pair<ProgPtr, std::pair<size_t, size_t>>> ct;
  std::vector<PsLaunch> rt;
  size_t mixed_off = 0, mixed_count = 0;  // tagged list (segment | erased << 30), count 0: none
  std::vector<uint8_t> mixed_e;  // the same erasures per segment in natural order (variant 90)
  struct FdLaunch {
    int side;           // 0, 1: syndrome-row decoder of that side; 2: formal derivative
    bool big;           // cec::fftdec_big of the plans' syndrome slot count
    size_t off, count;  // segments list + per-segment FFT-domain plans (pointer array)
  };
  std::vector<FdLaunch> fd;
};

constexpr size_t kDefaultDecodeCache = 4096;

}  // namespace

struct cec_codec {
  int k = 0, m = 0, device = 0;
  std::unique_ptr<BigMat> E;
  hipStream_t stream = nullptr;  // private: uploads and the host-buffer API
  KernelOpts opts;
  bool force_generic = false;
  // RS(32,32) patterns with at least this many outputs take the FFT-domain decoder (0: never)
  int fftdec_min = 4;
  int fftdec_mode = 0;  // 0: by the cost model (fftdec_choice), 1: syndrome rows, 2: derivative
  uint64_t fd_segments = 0;  // segments rebuilt by the FFT-domain decoders (CEC_STAT_FFTDEC_SEGMENTS)
  uint64_t fdd_segments = 0;  // of those, by the formal-derivative one (CEC_STAT_FFTDEC_D_SEGMENTS)
  DevPool pool;  // declared before every holder of pool blocks: destroyed after them
  ProgPtr encode;
  // decode programs by erasure pattern (n presence flags + data_only), least recently used last
  struct Entry {
    ProgPtr prog;
    std::list<std::string>::iterator lru;
  };
  std::unordered_map<std::string, Entry> decode_cache;
  std::list<std::string> lru;
  size_t cache_cap = kDefaultDecodeCache;
  std::unique_ptr<PsPlan> ps;
  // decode-plan scratch, reused pattern after pattern (a codec is not re-entrant): allocating
  // and zeroing these ~450 KB per new pattern was most of a new plan's host time
  struct PlanScratch {
    BigPlan plan;
    BigMat a, ainv, coef;
    WorkMat work;
  };
  std::unique_ptr<PlanScratch> scratch;
  PinnedArena arena;  // program images of a plan being built (uploads in flight)
  PlanScratch& plan_scratch() {
    if (!scratch) scratch = std::make_unique<PlanScratch>();
    return *scratch;
  }
  // staging for the host-buffer API: [n][stride]
  uint8_t* stage = nullptr;
  size_t stage_bytes = 0;

  void drop_plan() {
    if (!ps) return;
    pool.retire(ps->list, ps->list_bytes);
    pool.retire(ps->ptrs, ps->ptrs_bytes);
    ps.reset();
  }
  ~cec_codec() {
    (void)hipSetDevice(device);
    // no device-wide synchronisation: every launch that reads a pool block (a run-time encode
    // or decode program, a plan's arrays, audit indices) is followed by a mark on its stream, and
    // pool.drain() waits for those marks only; other codecs' streams keep running
    drop_plan();
    decode_cache.clear();
    lru.clear();
    encode.reset();
    pool.drain();
    if (stage) {
      (void)hipFreeAsync(stage, stream);  // the host API's calls synchronise before returning
      (void)hipStreamSynchronize(stream);
    }
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

// Batched calls run on the caller's stream; NULL is the HIP null (legacy default) stream, as
// in the HIP API itself (torch's default stream has handle 0).
hipStream_t pick_stream(cec_codec*, void* s) { return reinterpret_cast<hipStream_t>(s); }

Layout batch_layout(const cec_codec* c, const uint8_t* d_data, const uint8_t* d_parity,
                    size_t shard_len) {
  Layout L{};
  L.data = const_cast<uint8_t*>(d_data);
  L.parity = const_cast<uint8_t*>(d_parity);
  L.len = shard_len;
  L.shard_stride = shard_len;
  L.data_seg_stride = (uint64_t)c->k * shard_len;
  L.par_seg_stride = (uint64_t)c->m * shard_len;
  L.k = c->k;
  return L;
}

void launch_chunk(const KernelOpts& o, const Layout& L, const uint32_t* chunk,
                  const uint32_t* const* per_seg, int nin, int nob, const uint32_t* seg_list,
                  uint32_t nseg, hipStream_t st) {
  // bit-plane accumulators for one to four outputs from a wide input set (RS(32,32) rebuilds
  // vs k_rthx: one lost fragment 5.84 vs 4.03 TB/s, two 4.89 vs 3.75, three 3.89 vs 3.55, four
  // 3.36 vs 3.33; RS(10,4) encode 3.54 vs 3.41; bench.py --config 6 --erasures e / --config 8,
  // profiles/r02/rtb_sweep.txt)
  if (cec::rt_takes_rtb(o, nob, nin) &&
      cec::launch_matvec_rtb(L, chunk, per_seg, nob, seg_list, nseg, st, o.ct_variant))
    return;
  if (nin <= cec::kRthMaxIn &&
      cec::launch_matvec_rth(o, L, chunk, per_seg, nin, seg_list, nseg, st))
    return;
  cec::launch_matvec_rt(L, chunk, per_seg, nob, seg_list, nseg, st);
}

void run_program(const KernelOpts& o, const Program& p, const Layout& L, const uint32_t* seg_list,
                 uint32_t nseg, hipStream_t st) {
  for (const auto& c : p.chunks)
    launch_chunk(o, L, c.dev, nullptr, c.nin, c.nob, seg_list, nseg, st);
}

int do_encode(cec_codec* c, const Layout& L, const uint32_t* seg_list, uint32_t nseg,
              hipStream_t st) {
  if (nseg == 0 || L.len == 0) return CEC_OK;
  if (c->force_generic || !cec::launch_encode_ct(c->opts, c->k, c->m, L, seg_list, nseg, st)) {
    // the run-time program reads pool blocks (the encode program's chunks): mark the stream so
    // the codec's destruction waits for this launch (compile-time kernels read none)
    run_program(c->opts, *c->encode, L, seg_list, nseg, st);
    int rc = check_launch();
    return rc ? rc : c->pool.mark(st);
  }
  return check_launch();
}

int scratch_alloc(cec_codec* c, size_t bytes, hipStream_t st, Scratch* s) {
  s->bytes = bytes;
  if (bytes >= kBigScratch) {
    s->async = true;
    CEC_HIP_TRY(hipMallocAsync(&s->p, bytes, st));
    return CEC_OK;
  }
  return c->pool.alloc(bytes, &s->p);
}
// after the launches reading the scratch are enqueued (and, for a pool block, marked)
void scratch_release(cec_codec* c, const Scratch& s, hipStream_t st) {
  if (!s.p) return;
  if (s.async)
    (void)hipFreeAsync(s.p, st);
  else
    c->pool.retire(s.p, s.bytes);
}

// Cache keys start with a kind tag, so keys of different kinds never compare equal whatever
// their lengths: 'F' full rebuild, 'P' partial rebuild, 'R' rebuild of a required subset, 'W'
// partial rebuild of a wanted subset (decode LRU); 'S' / 'Q' / 'T' the per-segment plans of cec_reconstruct_batch /
// cec_reconstruct_partial_batch / cec_reconstruct_some_batch.
std::string pattern_key(const uint8_t* present, int n, bool data_only) {
  std::string key(n + 2, '\0');
  key[0] = 'F';
  for (int i = 0; i < n; ++i) key[1 + i] = present[i] ? 1 : 0;
  key[n + 1] = data_only ? 1 : 0;
  return key;
}

// Key of a partial rebuild: kind 'P', the pattern, then the held flags. With `required` (n flags;
// flags of present shards are ignored) only the lost shards it flags are outputs
// (cec_reconstruct_partial_ptrs): kind 'W' and the wanted flags behind the held ones, unless the
// subset names every lost shard, which is the 'P' entry of cec_reconstruct_partial_batch. `want`
// (n flags, may be null without `required`) receives the normalised subset.
std::string partial_key(const uint8_t* present, const uint8_t* held, int n, bool data_only,
                        int k = 0, const uint8_t* required = nullptr, uint8_t* want = nullptr) {
  std::string key = pattern_key(present, n, data_only);
  key[0] = 'P';
  for (int i = 0; i < n; ++i) key.push_back(held[i] ? 1 : 0);
  if (!required) return key;
  bool all = true;
  for (int i = 0; i < n; ++i) {
    const bool lost = !present[i] && !(data_only && i >= k);
    want[i] = lost && required[i] ? 1 : 0;
    if (lost && !want[i]) all = false;
  }
  if (all) return key;
  key[0] = 'W';
  for (int i = 0; i < n; ++i) key.push_back((char)want[i]);
  return key;
}

// Key of a rebuild of the lost shards flagged in `required` only (ReconstructSome; flags of
// present shards are ignored): kind 'R', the pattern, then the wanted flags. A subset that names
// every shard the full rebuild writes is the full rebuild and gets its 'F' key, so entries and keys
// of the calls without `required` are exactly what they were. `want` (n flags) receives the
// normalised subset.
std::string some_key(const uint8_t* present, const uint8_t* required, int k, int n,
                     bool data_only, uint8_t* want) {
  std::string key = pattern_key(present, n, data_only);
  bool all = true;
  for (int i = 0; i < n; ++i) {
    const bool lost = !present[i] && !(data_only && i >= k);
    want[i] = lost && (!required || required[i]) ? 1 : 0;
    if (lost && !want[i]) all = false;
  }
  if (all) return key;
  key[0] = 'R';
  for (int i = 0; i < n; ++i) key.push_back((char)want[i]);
  return key;
}

// The decode LRU. cache_find makes a hit the most recently used entry; nothing is evicted by
// cache_put: the caller evicts after its launches are enqueued and marked (evict_decode), so a
// program resolved earlier in the same call is never dropped under it.
ProgPtr cache_find(cec_codec* c, const std::string& key) {
  auto it = c->decode_cache.find(key);
  if (it == c->decode_cache.end()) return nullptr;
  c->lru.splice(c->lru.begin(), c->lru, it->second.lru);
  return it->second.prog;
}

void cache_put(cec_codec* c, std::string key, const ProgPtr& prog) {
  c->lru.push_front(key);
  c->decode_cache.emplace(std::move(key), cec_codec::Entry{prog, c->lru.begin()});
}

// Solve the erasure pattern `flags` (n flags of 0 / 1) of the code with encode matrix E into
// sc.plan: the rows that rebuild every lost shard from survivor_set's survivors (cec_survivors).
int solve_pattern(int k, int m, const BigMat& E, const uint8_t* flags, bool data_only,
                  cec_codec::PlanScratch& sc) {
  uint8_t rd[cec::kMaxShards];
  if (!cec::survivor_set(k, m, flags, rd) ||
      cec::gf_decode_plan_sys(k, m, flags, data_only, E, sc.plan, sc.a, sc.ainv, sc.work, rd) != 0)
    return set_err(CEC_ETOOFEW, "fewer than k shards present");
  return CEC_OK;
}

// Keep the rows of a solved plan whose outputs `want` flags (n flags), in their order.
void keep_wanted_rows(BigPlan* plan, const uint8_t* want, int k) {
  int w = 0;
  for (int o = 0; o < plan->nout; ++o) {
    if (!want[plan->out_idx[o]]) continue;
    if (w != o) {
      plan->out_idx[w] = plan->out_idx[o];
      std::memcpy(plan->coef.v[w], plan->coef.v[o], k);
    }
    ++w;
  }
  plan->nout = w;
  plan->coef.rows = w;
}

// Decode program for one erasure pattern (LRU-cached). With `required`, only the lost shards it
// flags are outputs (rows of the same decode: the survivors read do not change). `key_out`
// receives the pattern's cache key.
int get_decode(cec_codec* c, const uint8_t* present, bool data_only, ProgPtr* out,
               HostImages* keep = nullptr, const uint8_t* required = nullptr,
               std::string* key_out = nullptr) {
  const int n = c->k + c->m;
  uint8_t want[cec::kMaxShards];
  std::string key = required ? some_key(present, required, c->k, n, data_only, want)
                             : pattern_key(present, n, data_only);
  if (key_out) *key_out = key;
  const bool some = key[0] == 'R';
  if (some && !std::memchr(want, 1, n)) {
    // nothing asked for: nothing to do, whatever is present (klauspost returns before it counts
    // the shards)
    *out = std::make_shared<const Program>();
    return CEC_OK;
  }
  if ((*out = cache_find(c, key))) return CEC_OK;
  auto& sc = c->plan_scratch();
  auto* plan = &sc.plan;
  uint8_t flags[cec::kMaxShards];
  std::memcpy(flags, key.data() + 1, n);
  int rc = solve_pattern(c->k, c->m, *c->E, flags, data_only, sc);
  if (rc) return rc;
  if (some) keep_wanted_rows(plan, want, c->k);
  ProgPtr prog;
  if (plan->nout > 0) {
    // RS(32,32) rebuilds of several shards: also the FFT-domain plan (picked at launch by the
    // codec's CEC_OPT_FFTDEC_MIN and the layout)
    // They read exactly the program's survivors (the first k present shards): callers stage
    // only those (the host API below, the multi-GPU gathers), so the plans must not touch any
    // other shard flagged present.
    cec::FftDecPlan fdp, fddp;
    const bool wide = c->k == 32 && c->m == 32 && plan->nout >= 2;
    uint8_t read[cec::kMaxShards] = {};
    for (int j = 0; j < c->k; ++j) read[plan->in_idx[j]] = 1;
    const uint8_t* wf = some ? want : nullptr;  // the plans' output lists shrink to the subset
    const bool fd = wide && cec::fftdec_plan_m(read, flags, data_only, &fdp, wf);
    const bool fdd = wide && cec::fftdec_plan_d(read, flags, data_only, &fddp, wf);
    rc = build_program(c->pool, c->stream, plan->in_idx, c->k, plan->out_idx, plan->nout,
                       plan->coef, &prog, false, keep, fd ? &fdp : nullptr,
                       fdd ? &fddp : nullptr);
    if (rc) return rc;
  } else {
    prog = std::make_shared<const Program>();
  }
  cache_put(c, std::move(key), prog);
  *out = std::move(prog);
  return CEC_OK;
}

// Partial decode program (the partial-product exchange of SURVEY.md §8e): the decode rows of
// pattern `present` (survivors = survivor_set's, cec_survivors) restricted to the survivors flagged
// in `held`. The rebuild is linear in the survivors, so the XOR of the partials over any
// partition of the survivors is the full rebuild. No held survivor: a zero program (one input
// column with zero coefficients), so the outputs are still written (as zeros). Cached in the
// decode LRU under its own key, which `key_out` receives.
int get_partial(cec_codec* c, const uint8_t* present, const uint8_t* held, bool data_only,
                ProgPtr* out, HostImages* keep = nullptr, std::string* key_out = nullptr,
                const uint8_t* required = nullptr) {
  const int n = c->k + c->m;
  uint8_t want[cec::kMaxShards];
  std::string key = partial_key(present, held, n, data_only, c->k, required, want);
  if (key_out) *key_out = key;
  const bool some = key[0] == 'W';
  if (some && !std::memchr(want, 1, n)) {  // nothing asked for: nothing to do
    *out = std::make_shared<const Program>();
    return CEC_OK;
  }
  if ((*out = cache_find(c, key))) return CEC_OK;
  auto& sc = c->plan_scratch();
  auto* plan = &sc.plan;
  uint8_t flags[cec::kMaxShards];
  std::memcpy(flags, key.data() + 1, n);
  int rc = solve_pattern(c->k, c->m, *c->E, flags, data_only, sc);
  if (rc) return rc;
  if (some) keep_wanted_rows(plan, want, c->k);
  ProgPtr prog;
  if (plan->nout > 0) {
    uint8_t in_sub[cec::kMaxShards];
    int nsub = 0;
    auto* coef = &sc.coef;
    for (int o = 0; o < plan->nout; ++o) std::memset(coef->v[o], 0, sizeof coef->v[o]);
    for (int j = 0; j < c->k; ++j)
      if (held[plan->in_idx[j]]) {
        for (int o = 0; o < plan->nout; ++o) coef->v[o][nsub] = plan->coef.v[o][j];
        in_sub[nsub++] = plan->in_idx[j];
      }
    if (nsub == 0) {  // zero program: one column, zero coefficients (cleared above)
      in_sub[0] = plan->in_idx[0];
      nsub = 1;
    }
    rc = build_program(c->pool, c->stream, in_sub, nsub, plan->out_idx, plan->nout, *coef, &prog,
                       true, keep);
    if (rc) return rc;
  } else {
    prog = std::make_shared<const Program>();
  }
  cache_put(c, std::move(key), prog);
  *out = std::move(prog);
  return CEC_OK;
}

// Drop least recently used patterns beyond the cap. A dropped program that a cached per-segment
// plan still uses stays alive through the plan; device blocks are retired, not freed.
void evict_decode(cec_codec* c) {
  while (c->decode_cache.size() > c->cache_cap && !c->lru.empty()) {
    c->decode_cache.erase(c->lru.back());
    c->lru.pop_back();
  }
}

// "Every data shard present, every parity shard lost" is the encode itself: the compile-time
// encode kernels (RS(32,32): the additive FFT, 5.8 TB/s) rebuild it, not a run-time program of m
// outputs (k_rthx, ~2.7 TB/s at 32).
bool is_reencode(const cec_codec* c, const Program& p) {
  if (p.partial || p.nout != c->m) return false;
  for (int o = 0; o < p.nout; ++o)
    if (p.out_idx[o] != c->k + o) return false;
  for (int j = 0; j < c->k; ++j)
    if (p.in_idx[j] != j) return false;
  return true;
}

// The decoder choice per pattern and per batch: fftdec_cost.h (tested on CPU against the
// recorded warm sweep, tests/test_host.py::test_fftdec_chooser_on_recorded_costs).
using cec::kFdD;
using cec::kFdM;
using cec::kFdNone;

// tuning build: CEC_OPT_CT_VARIANT 70 runs the pipelined persistent k_fftdec_dp instead of the
// one-block-per-wave k_fftdec_d, 72 the same with wave priorities, 73 k_fftdec_d with its quad
// exchanges through the LDS crossbar, 74..78 that in some phases only: the derivative, IFFT +
// derivative, the FFT tail, the IFFT, derivative + tail; 83 DPP in every phase (= the product's);
// 85 the product's without the skip of unread input slots (A/B sweeps)
// tuning build: CEC_OPT_CT_VARIANT 79..82 run k_fftdec_m with pair exchanges through the LDS
// crossbar: the IFFT's; + the FFT's last layer; + the nibble packs; all three; 84 DPP everywhere
// (= the product's). launch_fftdec's form is 1 + that mask; 86 (form 10) the product's without
// the skip of unread input slots.
int fdm_form(const cec_codec* c) {
  switch (c->opts.ct_variant) {
    case 79: return 2;
    case 80: return 4;
    case 81: return 6;
    case 82: return 8;
    case 84: return 1;
    case 86: return 10;
    default: return 0;
  }
}

int fdd_form(const cec_codec* c) {
  switch (c->opts.ct_variant) {
    case 70: return 1;
    case 72: return 3;
    case 73: return 4;
    case 74: return 5;
    case 75: return 6;
    case 76: return 7;
    case 77: return 8;
    case 78: return 9;
    case 83: return 10;
    case 85: return 11;
    default: return 0;
  }
}

int use_fftdec(const cec_codec* c, const Program& p) {
  if (c->force_generic || (!p.fd && !p.fdd) || c->fftdec_min <= 0 || p.nout < c->fftdec_min)
    return kFdNone;
  if (c->fftdec_mode == 1) return p.fd ? kFdM : kFdNone;
  if (c->fftdec_mode == 2) return p.fdd ? kFdD : kFdNone;
  return cec::fftdec_choice(p.nout, p.fd_nrs, cec::fftdec_big(p.fd_nrs), p.fd != nullptr,
                            p.fdd != nullptr);
}

int do_decode(cec_codec* c, const Program& p, const Layout& L, const uint32_t* seg_list,
              uint32_t nseg, hipStream_t st) {
  if (p.nout == 0 || nseg == 0 || L.len == 0) return CEC_OK;
  if (!c->force_generic && p.single < 0 && is_reencode(c, p))
    return do_encode(c, L, seg_list, nseg, st);
  const int fk = use_fftdec(c, p);
  if ((fk == kFdM && cec::launch_fftdec(L, p.fd_side, cec::fftdec_big(p.fd_nrs), p.fd, nullptr,
                                        seg_list, nseg, st, fdm_form(c))) ||
      (fk == kFdD && cec::launch_fftdec_d(L, p.fdd, nullptr, seg_list, nseg, st, fdd_form(c)))) {
    c->fd_segments += nseg;
    if (fk == kFdD) c->fdd_segments += nseg;
    return check_launch();
  }
  if (c->force_generic || p.single < 0 ||
      !cec::launch_decode_ct(c->opts, c->k, c->m, p.single, L, seg_list, nseg, st))
    run_program(c->opts, p, L, seg_list, nseg, st);
  return check_launch();
}

// Grow a buffer used only on stream `st` (stream-ordered: no device-wide synchronisation).
int ensure(uint8_t** buf, size_t* have, size_t need, hipStream_t st) {
  if (*have >= need) return CEC_OK;
  if (*buf) (void)hipFreeAsync(*buf, st);
  *buf = nullptr;
  *have = 0;
  CEC_HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(buf), need, st));
  *have = need;
  return CEC_OK;
}

size_t pad256(size_t x) { return (x + 255) & ~size_t(255); }

// Host-buffer API staging layout: one segment, shards at stride pad256(len).
Layout stage_layout(cec_codec* c, size_t len) {
  const size_t stride = pad256(len);
  Layout L{};
  L.data = c->stage;
  L.parity = c->stage + (size_t)c->k * stride;
  L.len = len;
  L.shard_stride = stride;
  L.data_seg_stride = (uint64_t)(c->k + c->m) * stride;
  L.par_seg_stride = (uint64_t)(c->k + c->m) * stride;
  L.k = c->k;
  return L;
}

// The host-buffer calls: room for `nshards` staged shards of `len` bytes, and the copies of the
// `count` shards host[0..count) up to consecutive stage slots from `dev`, or down from them, on
// the codec's stream (the caller synchronises once, at the end).
int stage_ensure(cec_codec* c, size_t nshards, size_t len) {
  return ensure(&c->stage, &c->stage_bytes, pad256(len) * nshards, c->stream);
}
int stage_up(cec_codec* c, uint8_t* dev, const uint8_t* const* host, int count, size_t len) {
  for (int i = 0; i < count; ++i)
    CEC_HIP_TRY(hipMemcpyAsync(dev + i * pad256(len), host[i], len, hipMemcpyHostToDevice,
                               c->stream));
  return CEC_OK;
}
int stage_down(cec_codec* c, uint8_t* const* host, const uint8_t* dev, int count, size_t len) {
  for (int i = 0; i < count; ++i)
    CEC_HIP_TRY(hipMemcpyAsync(host[i], dev + i * pad256(len), len, hipMemcpyDeviceToHost,
                               c->stream));
  return CEC_OK;
}

// New patterns' program uploads stay in flight until one synchronisation per call (not per
// pattern: 64 new RS(32,32) patterns cost ~1 ms of waits otherwise); every return path waits for
// them before their host images go.
struct Uploads {
  hipStream_t st;
  PinnedArena& arena;
  ~Uploads() {
    if (arena.busy()) (void)hipStreamSynchronize(st);
    arena.reset();
  }
};

// What a per-segment plan rebuilds, and so what its pattern array `pkey` holds per segment: kFull
// n presence flags (cec_reconstruct_batch); kPartial n presence then n held flags, the programs
// partial (cec_reconstruct_partial_batch); kSome n presence then n required flags, the programs
// writing the required lost shards only (cec_reconstruct_some_batch).
enum PsKind { kFull, kPartial, kSome };

// Build the plan of a per-segment reconstruct for the pattern array `pkey` (a kind tag, the flags
// of nseg segments, then the options the plan depends on) into *out; device arrays are uploaded
// and complete on return. fdok: the layout fits the FFT-domain decoders (never for kPartial).
int build_ps_plan(cec_codec* c, const std::string& pkey, size_t nseg, PsKind kind, bool data_only,
                  bool fdok, size_t shard_len, std::unique_ptr<PsPlan>* out) {
  const int n = c->k + c->m;
  const int per = kind == kFull ? n : 2 * n;
  auto plan = std::make_unique<PsPlan>();
  plan->key = pkey;
  // group segments by pattern, in first-appearance order (deterministic launch order)
  std::unordered_map<std::string, size_t> gidx;
  std::vector<std::pair<std::string, std::vector<uint32_t>>> groups;
  for (size_t s = 0; s < nseg; ++s) {
    std::string k = pkey.substr(1 + s * per, per);
    auto it = gidx.find(k);
    if (it == gidx.end()) {
      it = gidx.emplace(k, groups.size()).first;
      groups.push_back({k, {}});
    }
    groups[it->second].second.push_back((uint32_t)s);
  }
  bool all_ct = !c->force_generic;
  std::vector<std::pair<ProgPtr, const std::vector<uint32_t>*>> progs, reencode, fdg[5];
  Uploads up{c->stream, c->arena};  // synchronised once, below
  for (auto& g : groups) {
    ProgPtr p;
    std::string key;
    const uint8_t* flags = reinterpret_cast<const uint8_t*>(g.first.data());
    int rc = kind == kPartial
                 ? get_partial(c, flags, flags + n, data_only, &p, &up.arena, &key)
                 : get_decode(c, flags, data_only, &p, &up.arena,
                              kind == kSome ? flags + n : nullptr, &key);
    if (rc) return rc;
    plan->keys.push_back(std::move(key));
    if (!p->nout) continue;
    plan->progs.push_back(p);
    if (!c->force_generic && p->single < 0 && is_reencode(c, *p)) {
      reencode.push_back({p, &g.second});  // the encode kernels, whatever the other groups take
      continue;
    }
    const int fk = fdok ? use_fftdec(c, *p) : kFdNone;
    if (fk == kFdM) {  // RS(32,32) wide rebuilds: the FFT-domain decoders
      fdg[p->fd_side * 2 + (cec::fftdec_big(p->fd_nrs) ? 1 : 0)].push_back({p, &g.second});
      continue;
    }
    if (fk == kFdD) {
      fdg[4].push_back({p, &g.second});
      continue;
    }
    progs.push_back({p, &g.second});
    if (p->single < 0 || !cec::has_decode_ct(c->k, c->m, p->single)) all_ct = false;
  }
  // The cost model picks per pattern; a batch whose patterns land on both decoders runs one more
  // launch than all-derivative. Fold the syndrome-row groups into the derivative launch when the
  // whole batch is cheaper that way (costs per segment scaled from 64 x 512 KiB).
  if (!fdg[4].empty() && c->fftdec_mode == 0) {
    std::vector<cec::FdmGroup> mg;
    int mlaunches = 0;
    for (int cls = 0; cls < 4; ++cls) {
      if (fdg[cls].empty()) continue;
      ++mlaunches;
      for (auto& pr : fdg[cls]) {
        const Program& q = *pr.first;
        mg.push_back({pr.second->size(), q.nout, q.fd_nrs, cec::fftdec_big(q.fd_nrs),
                      q.fdd != nullptr});
      }
    }
    if (cec::fftdec_fold(mg, mlaunches, shard_len)) {
      for (int cls = 0; cls < 4; ++cls) {
        for (auto& pr : fdg[cls]) fdg[4].push_back(pr);
        fdg[cls].clear();
      }
    }
  }
  std::vector<uint32_t> hl;
  std::vector<const uint32_t*> hp;
  for (auto& pr : reencode) {
    plan->ct.push_back({pr.first, {hl.size(), pr.second->size()}});
    hl.insert(hl.end(), pr.second->begin(), pr.second->end());
  }
  // the run-time launches index the segment list and the chunk-pointer array with one offset:
  // keep them aligned past the re-encode lists
  hp.resize(hl.size(), nullptr);
  for (int cls = 0; cls < 5; ++cls) {  // side x size class, and the derivative: one launch each
    if (fdg[cls].empty()) continue;
    PsPlan::FdLaunch f{cls == 4 ? 2 : cls >> 1, (cls & 1) != 0, hl.size(), 0};
    for (auto& pr : fdg[cls])
      for (uint32_t sg : *pr.second) {
        hl.push_back(sg);
        hp.push_back(cls == 4 ? pr.first->fdd : pr.first->fd);
        ++f.count;
      }
    plan->fd.push_back(f);
  }
  if (all_ct) {
    std::vector<uint32_t> tagged;
    for (auto& pr : progs) {
      plan->ct.push_back({pr.first, {hl.size(), pr.second->size()}});
      hl.insert(hl.end(), pr.second->begin(), pr.second->end());
      for (uint32_t sg : *pr.second) tagged.push_back(sg | ((uint32_t)pr.first->single << 30));
    }
    if (c->k == 2 && c->m == 1 && plan->ct.size() > 1 && nseg < (1u << 30)) {
      // grouped by erasure pattern, not in segment order: the workgroups resident at once then
      // mostly share one pattern (config 3, erased = seg mod 3: 0.253 -> 0.250 ms per GiB batch;
      // a uniform pattern takes 0.244-0.248, bench.py --erase)
      plan->mixed_off = hl.size();
      plan->mixed_count = tagged.size();
      hl.insert(hl.end(), tagged.begin(), tagged.end());
      // tuning variant 90's per-row codes: the lost shard of a tagged segment, 3 = untouched (an
      // intact segment, or one another launch handles: nothing is written to it)
      plan->mixed_e.assign(nseg, 3);
      for (uint32_t w : tagged) plan->mixed_e[w & 0x3FFFFFFFu] = (uint8_t)(w >> 30);
    }
  } else {
    size_t maxchunks = 0;
    for (auto& pr : progs) maxchunks = std::max(maxchunks, pr.first->chunks.size());
    for (size_t ci = 0; ci < maxchunks; ++ci) {
      std::vector<std::pair<int, std::vector<std::pair<uint32_t, const uint32_t*>>>> byb;
      int nin_max = 0;
      for (auto& pr : progs)
        if (ci < pr.first->chunks.size()) {
          const RtChunk& ch = pr.first->chunks[ci];
          nin_max = std::max(nin_max, ch.nin);
          auto it = std::find_if(byb.begin(), byb.end(),
                                 [&](const auto& b) { return b.first == ch.nob; });
          if (it == byb.end()) it = byb.insert(byb.end(), {ch.nob, {}});
          for (uint32_t sg : *pr.second) it->second.push_back({sg, ch.dev});
        }
      for (auto& b : byb) {
        PsLaunch l;
        l.nob = b.first;
        l.nin = nin_max;
        l.off = hl.size();
        l.count = b.second.size();
        for (auto& e : b.second) {
          hl.push_back(e.first);
          hp.push_back(e.second);
        }
        plan->rt.push_back(l);
      }
    }
  }
  void* d = nullptr;
  plan->list_bytes = std::max<size_t>(hl.size(), 1) * sizeof(uint32_t);
  int rc = c->pool.alloc(plan->list_bytes, &d);
  if (rc) return rc;
  plan->list = static_cast<uint32_t*>(d);
  plan->ptrs_bytes = std::max<size_t>(hp.size(), 1) * sizeof(void*);
  rc = c->pool.alloc(plan->ptrs_bytes, &plan->ptrs);
  if (rc) {
    c->pool.retire(plan->list, plan->list_bytes);
    return rc;
  }
  hipError_t e = hipSuccess;
  if (!hl.empty())
    e = hipMemcpyAsync(plan->list, hl.data(), hl.size() * sizeof(uint32_t),
                       hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && !hp.empty())
    e = hipMemcpyAsync(plan->ptrs, hp.data(), hp.size() * sizeof(void*), hipMemcpyHostToDevice,
                       c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the programs' uploads too
  if (e != hipSuccess) {
    c->pool.retire(plan->list, plan->list_bytes);
    c->pool.retire(plan->ptrs, plan->ptrs_bytes);
    return set_err(CEC_EHIP, std::string("plan upload: ") + hipGetErrorString(e));
  }
  up.arena.reset();  // its uploads have landed
  *out = std::move(plan);
  return CEC_OK;
}

int launch_ps_plan(cec_codec* c, const PsPlan& p, const Layout& L, hipStream_t st) {
  if (p.mixed_count && c->opts.ct_variant == 90 &&
      cec::launch_decode1_mixed_kargs(c->k, c->m, L, p.mixed_e.data(),
                                      (uint32_t)p.mixed_e.size(), st))
    return check_launch();
  if (p.mixed_count &&
      cec::launch_decode1_mixed(c->opts, c->k, c->m, L, p.list + p.mixed_off,
                                (uint32_t)p.mixed_count, st))
    return check_launch();
  for (const auto& w : p.ct) {
    int rc = do_decode(c, *w.first, L, p.list + w.second.first, (uint32_t)w.second.second, st);
    if (rc) return rc;
  }
  const uint32_t* const* ptrs = static_cast<const uint32_t* const*>(p.ptrs);
  for (const auto& f : p.fd) {
    const bool ok = f.side == 2 ? cec::launch_fftdec_d(L, nullptr, ptrs + f.off, p.list + f.off,
                                                       (uint32_t)f.count, st, fdd_form(c))
                                : cec::launch_fftdec(L, f.side, f.big, nullptr, ptrs + f.off,
                                                     p.list + f.off, (uint32_t)f.count, st,
                                                     fdm_form(c));
    if (!ok)
      return set_err(CEC_EINVAL, "FFT-domain decode plan on a layout it does not fit");
    c->fd_segments += f.count;
    if (f.side == 2) c->fdd_segments += f.count;
    int rc = check_launch();
    if (rc) return rc;
  }
  for (const auto& l : p.rt) {
    launch_chunk(c->opts, L, nullptr, ptrs + l.off, l.nin, l.nob, p.list + l.off,
                 (uint32_t)l.count, st);
    int rc = check_launch();
    if (rc) return rc;
  }
  return CEC_OK;
}

// A per-segment reconstruct: the codec's cached plan when `pkey` repeats (degraded-read and repair
// loops pass the same map each call), else a new one; then its launches and their mark.
int run_ps_plan(cec_codec* c, const std::string& pkey, size_t nseg, PsKind kind, bool data_only,
                bool fdok, size_t shard_len, const Layout& L, hipStream_t st) {
  if (!c->ps || c->ps->key != pkey) {
    std::unique_ptr<PsPlan> plan;
    int rc = build_ps_plan(c, pkey, nseg, kind, data_only, fdok, shard_len, &plan);
    if (rc) return rc;
    c->drop_plan();  // the old plan's arrays are retired: launches already enqueued keep them
    c->ps = std::move(plan);
  } else {
    for (const auto& key : c->ps->keys) (void)cache_find(c, key);  // they stay recently used
  }
  const int rc = launch_ps_plan(c, *c->ps, L, st);
  // completion point of these launches; only then may evicted programs be retired
  const int mrc = c->pool.mark(st);
  evict_decode(c);
  return rc ? rc : mrc;
}

// The opening checks of the batched calls, after their null tests.
int check_batch(size_t nseg, size_t shard_len) {
  if (shard_len == 0) return set_err(CEC_ESHARDLEN, "zero shard length");
  if (nseg > 0xffffffffull) return set_err(CEC_EINVAL, "too many segments");
  return CEC_OK;
}

}  // namespace

namespace cec {
// error reporting shared with hashq.cpp (same thread-local detail string)
int set_error(int code, const std::string& msg) { return set_err(code, msg); }
}  // namespace cec

extern "C" {

const char* cec_version(void) {
#ifdef CEC_TUNING
  return "cessec 0.2.0 gfx950 tuning";
#else
  return "cessec 0.2.0 gfx950";
#endif
}

const char* cec_strerror(int code) {
  switch (code) {
    case CEC_OK: return "ok";
    case CEC_EINVAL: return "invalid argument";
    case CEC_ETOOFEW: return "too few shards given";
    case CEC_ESHARDLEN: return "shard sizes do not match";
    case CEC_EHIP: return "HIP runtime error";
    case CEC_ENOMEM: return "out of memory";
    case CEC_ENCCL: return "RCCL error";
    case CEC_ESHORTDATA: return "not enough data to fill the number of requested shards";
    case CEC_ENODEV: return "no GPU device";
    case CEC_ESEGCOUNT: return "file exceeds SegmentCount segments";
    case CEC_ECALLBACK: return "callback failed";
  }
  return "unknown error";
}

const char* cec_last_error(void) { return g_last_error.c_str(); }

int cec_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int cec_create(int k, int m, int device, cec_codec** out) {
  if (!out) return set_err(CEC_EINVAL, "null out");
  *out = nullptr;
  if (k < 1 || m < 1 || k + m > cec::kMaxShards)
    return set_err(CEC_EINVAL, "need k >= 1, m >= 1, k + m <= 256");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return set_err(CEC_ENODEV, "no HIP device visible");
  if (device < 0 || device >= ndev) return set_err(CEC_EINVAL, "device index out of range");
  CEC_HIP_TRY(hipSetDevice(device));
  std::unique_ptr<cec_codec> c(new (std::nothrow) cec_codec);
  if (!c) return set_err(CEC_ENOMEM, "codec");
  c->k = k;
  c->m = m;
  c->device = device;
  c->E = std::make_unique<BigMat>();
  {
    auto top = std::make_unique<BigMat>();
    auto topinv = std::make_unique<BigMat>();
    auto work = std::make_unique<WorkMat>();
    if (!cec::gf_encode_matrix(k, m, *c->E, *top, *topinv, *work))
      return set_err(CEC_EINVAL, "singular Vandermonde top block");
  }
  CEC_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->pool.set_stream(c->stream);
  {
    auto par = std::make_unique<BigMat>();
    uint8_t in_idx[cec::kMaxShards], out_idx[cec::kMaxShards];
    for (int j = 0; j < k; ++j) in_idx[j] = (uint8_t)j;
    for (int o = 0; o < m; ++o) {
      out_idx[o] = (uint8_t)(k + o);
      for (int j = 0; j < k; ++j) par->v[o][j] = c->E->v[k + o][j];
    }
    int rc = build_program(c->pool, c->stream, in_idx, k, out_idx, m, *par, &c->encode);
    if (rc) return rc;
  }
  *out = c.release();
  return CEC_OK;
}

void cec_destroy(cec_codec* codec) { delete codec; }

int cec_codec_info(const cec_codec* c, int* k, int* m, int* device) {
  if (!c) return set_err(CEC_EINVAL, "null codec");
  if (k) *k = c->k;
  if (m) *m = c->m;
  if (device) *device = c->device;
  return CEC_OK;
}

int cec_matrix(const cec_codec* c, uint8_t* out) {
  if (!c || !out) return set_err(CEC_EINVAL, "null");
  for (int r = 0; r < c->k + c->m; ++r)
    for (int j = 0; j < c->k; ++j) out[r * c->k + j] = c->E->v[r][j];
  return CEC_OK;
}

int cec_set_option(cec_codec* c, int option, int value) {
  if (!c) return set_err(CEC_EINVAL, "null codec");
  switch (option) {
    case CEC_OPT_FORCE_GENERIC:
      c->force_generic = value != 0;
      return CEC_OK;
    case CEC_OPT_CT_VARIANT:
      if (value < -1 || value > cec::max_ct_variant())
        return set_err(CEC_EINVAL, cec::max_ct_variant() == 0
                                       ? "kernel variants need the tuning build (libcessec_tune)"
                                       : "variant out of range");
      c->opts.ct_variant = value == 0 && cec::max_ct_variant() == 0 ? -1 : value;
      return CEC_OK;
    case CEC_OPT_SHA_MODE:
      if (value < 0 || value > 3) return set_err(CEC_EINVAL, "sha mode out of range");
      c->opts.sha_mode = value;
      return CEC_OK;
    case CEC_OPT_RT_MODE:
      if (value < 0 || value > 3) return set_err(CEC_EINVAL, "rt mode out of range");
      c->opts.rt_mode = value;
      return CEC_OK;
    case CEC_OPT_FFTDEC_MIN:
      if (value < 0 || value > 64) return set_err(CEC_EINVAL, "fftdec min outputs in 0..64");
      c->fftdec_min = value;
      return CEC_OK;
    case CEC_OPT_FFTDEC_MODE:
      if (value < 0 || value > 2)
        return set_err(CEC_EINVAL, "fftdec mode is 0 (auto), 1 (syndrome rows) or 2 (derivative)");
      c->fftdec_mode = value;
      return CEC_OK;
    case CEC_OPT_DECODE_CACHE:
      if (value < 1) return set_err(CEC_EINVAL, "decode cache capacity must be >= 1");
      c->cache_cap = (size_t)value;
      evict_decode(c);
      return CEC_OK;
  }
  return set_err(CEC_EINVAL, "unknown option");
}

int cec_get_stat(const cec_codec* c, int stat, uint64_t* value) {
  if (!c || !value) return set_err(CEC_EINVAL, "null");
  switch (stat) {
    case CEC_STAT_DECODE_CACHED: *value = c->decode_cache.size(); return CEC_OK;
    case CEC_STAT_RETIRED_PENDING: *value = c->pool.pending(); return CEC_OK;
    case CEC_STAT_POOL_BYTES: *value = c->pool.held(); return CEC_OK;
    case CEC_STAT_FFTDEC_SEGMENTS: *value = c->fd_segments; return CEC_OK;
    case CEC_STAT_FFTDEC_D_SEGMENTS: *value = c->fdd_segments; return CEC_OK;
  }
  return set_err(CEC_EINVAL, "unknown stat");
}

int cec_encode_batch(cec_codec* c, const uint8_t* d_data, uint8_t* d_parity, size_t nseg,
                     size_t shard_len, void* hip_stream) {
  if (!c || (nseg && (!d_data || !d_parity))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(nseg, shard_len)) return rc;
  CEC_HIP_TRY(hipSetDevice(c->device));
  Layout L = batch_layout(c, d_data, d_parity, shard_len);
  return do_encode(c, L, nullptr, (uint32_t)nseg, pick_stream(c, hip_stream));
}

// cec_reconstruct_batch (required == NULL) and cec_reconstruct_some_batch (required: the same
// shape as present).
static int reconstruct_batch_impl(cec_codec* c, uint8_t* d_data, uint8_t* d_parity, size_t nseg,
                                  size_t shard_len, const uint8_t* present,
                                  const uint8_t* required, int per_segment, int data_only,
                                  void* hip_stream) {
  if (!c || !present || (nseg && (!d_data || !d_parity))) return set_err(CEC_EINVAL, "null");
  int rc = check_batch(nseg, shard_len);
  if (rc) return rc;
  CEC_HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, hip_stream);
  const int n = c->k + c->m;
  Layout L = batch_layout(c, d_data, d_parity, shard_len);
  if (per_segment) {
    // Per-segment patterns. Segments are grouped by pattern once and the plan is cached for a
    // repeated pattern array:
    //  * every pattern has a compile-time single-erasure kernel (RS(2,1)): one mixed-pattern
    //    launch (or one launch per pattern over its segment list);
    //  * otherwise: one multi-pattern run-time launch per (chunk index, bucket), each segment's
    //    workgroup row reading its own pattern's chunk, so a batch where every segment has a
    //    different erasure map is still one full-grid launch.
    std::string pkey(1, required ? 'T' : 'S');
    pkey.reserve(nseg * n * (required ? 2 : 1) + 16);
    if (!required) {
      for (size_t i = 0; i < nseg * n; ++i) pkey.push_back(present[i] ? 1 : 0);
    } else {  // per segment: n presence flags, then n required flags
      for (size_t s = 0; s < nseg; ++s) {
        for (int i = 0; i < n; ++i) pkey.push_back(present[s * n + i] ? 1 : 0);
        for (int i = 0; i < n; ++i) pkey.push_back(required[s * n + i] ? 1 : 0);
      }
    }
    pkey.push_back(data_only ? 1 : 0);
    pkey.push_back(c->force_generic ? 1 : 0);
    const bool fdok = cec::fftdec_layout_ok(L);
    pkey.push_back(fdok ? 1 : 0);
    pkey.push_back((char)c->fftdec_min);
    pkey.push_back((char)c->fftdec_mode);
    for (int b = 0; b < 8; ++b) pkey.push_back((char)(shard_len >> (8 * b)));  // the split rule
    return run_ps_plan(c, pkey, nseg, required ? kSome : kFull, data_only != 0, fdok, shard_len, L,
                       st);
  }
  ProgPtr p;
  rc = get_decode(c, present, data_only != 0, &p, nullptr, required);
  if (rc) return rc;
  rc = do_decode(c, *p, L, nullptr, (uint32_t)nseg, st);
  // completion point of these launches; only then may evicted programs be retired
  int mrc = c->pool.mark(st);
  evict_decode(c);
  return rc ? rc : mrc;
}

int cec_reconstruct_batch(cec_codec* c, uint8_t* d_data, uint8_t* d_parity, size_t nseg,
                          size_t shard_len, const uint8_t* present, int per_segment,
                          int data_only, void* hip_stream) {
  return reconstruct_batch_impl(c, d_data, d_parity, nseg, shard_len, present, nullptr,
                                per_segment, data_only, hip_stream);
}

int cec_reconstruct_some_batch(cec_codec* c, uint8_t* d_data, uint8_t* d_parity, size_t nseg,
                               size_t shard_len, const uint8_t* present, const uint8_t* required,
                               int per_segment, void* hip_stream) {
  if (!required) return set_err(CEC_EINVAL, "null");
  return reconstruct_batch_impl(c, d_data, d_parity, nseg, shard_len, present, required,
                                per_segment, 0, hip_stream);
}

int cec_decode_rows(int k, int m, const uint8_t* present, const uint8_t* required, uint8_t* rows,
                    uint8_t* out_idx, int* nreq) {
  if (!present || !required || !rows || !out_idx || !nreq) return set_err(CEC_EINVAL, "null");
  if (k < 1 || m < 1 || k + m > cec::kMaxShards)
    return set_err(CEC_EINVAL, "need k >= 1, m >= 1, k + m <= 256");
  const int n = k + m;
  auto E = std::make_unique<BigMat>();
  auto sc = std::make_unique<cec_codec::PlanScratch>();
  const BigPlan* plan = &sc->plan;
  if (!cec::gf_encode_matrix(k, m, *E, sc->a, sc->ainv, sc->work))
    return set_err(CEC_EINVAL, "singular Vandermonde top block");
  uint8_t flags[cec::kMaxShards];
  for (int i = 0; i < n; ++i) flags[i] = present[i] ? 1 : 0;
  if (int rc = solve_pattern(k, m, *E, flags, false, *sc)) return rc;
  int w = 0;
  for (int o = 0; o < plan->nout; ++o) {  // out_idx ascending, survivors in cec_survivors order
    if (!required[plan->out_idx[o]]) continue;
    out_idx[w] = plan->out_idx[o];
    std::memcpy(rows + (size_t)w * k, plan->coef.v[o], k);
    ++w;
  }
  *nreq = w;
  return CEC_OK;
}

// The pointer-table calls. Everything is validated and every program resolved before the first
// launch; the table is built on the host from the caller's arrays (which are not read after the
// return), uploaded to a pool block on the codec's stream and complete before the launches, and
// retired in stream order behind them.

// One kernel launch of such a call and its rows of the table.
enum class PtrKind {
  rs21,      // RS(2,1), compile-time coefficients
  bitplane,  // run-time program, the bit-plane product where the bucket has one (k_rtb's cases)
  masks,     // run-time program, the per-bit mask product
  xor_rows,  // cec_xor_ptrs
  acc        // parity accumulation (acc_ptrs_impl; never merged: see id)
};
struct PtrLaunch {
  PtrKind kind;
  int nob;
  uint32_t rs;
  std::vector<uint64_t> rows;
  int id = 0;  // acc: the launch's entry in the call's list of coefficient sets
};

static PtrLaunch& ptr_launch_of(std::vector<PtrLaunch>& launches, PtrKind kind, int nob,
                                uint32_t rs) {
  for (auto& l : launches)
    if (l.kind == kind && l.nob == nob && l.rs == rs) return l;
  launches.push_back({kind, nob, rs, {}});
  return launches.back();
}

// The kernel of an rs21 / bitplane / masks launch over its `nrows` rows at `tab`, with what `sink`
// does at the rows' output positions (`d_ok`: the compare's flags).
static void launch_ptr_rows(const PtrLaunch& l, cec::PtrSink sink, const uint64_t* tab,
                            uint32_t nrows, size_t shard_len, bool vec_ok, uint8_t* d_ok,
                            hipStream_t st) {
  if (l.kind == PtrKind::rs21)
    cec::launch_ptrs_rs21(sink, tab, nrows, shard_len, vec_ok, d_ok, st);
  else
    cec::launch_ptrs_rt(sink, l.kind == PtrKind::bitplane, tab, nrows, l.rs, l.nob, shard_len,
                        vec_ok, d_ok, st);
}

// Segments of a call grouped by a key string: the index of the key's group among the call's
// `ngroups` groups, or ngroups for a key not seen before, whose group the caller then appends.
static size_t group_of(std::unordered_map<std::string, size_t>& gidx, const std::string& key,
                       size_t ngroups) {
  const auto it = gidx.find(key);
  return it != gidx.end() ? it->second : gidx.emplace(key, ngroups).first->second;
}

// The RS(2,1) rows {input 0, input 1, output, case} of program p (one lost shard: p.single) for
// the segments `segs`; with `seg_word` the segment index rides in the case word's high half.
static void add_rs21_rows(const cec_codec* c, std::vector<PtrLaunch>& launches, const Program& p,
                          const std::vector<uint32_t>& segs, const uint8_t* const* src,
                          uint8_t* const* dst, bool seg_word) {
  const int n = c->k + c->m;
  PtrLaunch& l = ptr_launch_of(launches, PtrKind::rs21, 1, 4);
  for (uint32_t s : segs) {
    l.rows.push_back((uint64_t)(uintptr_t)src[(size_t)s * n + p.in_idx[0]]);
    l.rows.push_back((uint64_t)(uintptr_t)src[(size_t)s * n + p.in_idx[1]]);
    l.rows.push_back((uint64_t)(uintptr_t)dst[(size_t)s * n + p.out_idx[0]]);
    l.rows.push_back((uint64_t)p.out_idx[0] | (seg_word ? (uint64_t)s << 32 : 0));
  }
}

// The run-time rows of program p for the segments `segs`: per chunk and segment one row {program
// chunk, nin inputs, nout outputs} in the launch of the chunk's kernel and bucket, the addresses
// taken from the segment's n entries of src and dst. With `seg_word` the rows are one word longer
// and hold the segment index in their last word (the compare forms).
static void add_rt_rows(const cec_codec* c, std::vector<PtrLaunch>& launches, const Program& p,
                        const std::vector<uint32_t>& segs, const uint8_t* const* src,
                        uint8_t* const* dst, bool seg_word) {
  const int n = c->k + c->m;
  int o0 = 0;
  for (const RtChunk& ch : p.chunks) {
    const bool rtb = cec::rt_takes_rtb(c->opts, ch.nob, ch.nin);  // as launch_chunk
    PtrLaunch& l = ptr_launch_of(launches, rtb && ch.nob <= 4 ? PtrKind::bitplane : PtrKind::masks,
                                 ch.nob, (uint32_t)(1 + ch.nin + ch.nob + (seg_word ? 1 : 0)));
    for (uint32_t s : segs) {
      const size_t r0 = l.rows.size();
      l.rows.resize(r0 + l.rs, 0);
      uint64_t* r = l.rows.data() + r0;
      if (seg_word) r[l.rs - 1] = s;
      r[0] = (uint64_t)(uintptr_t)ch.dev;
      for (int j = 0; j < ch.nin; ++j) r[1 + j] = (uint64_t)(uintptr_t)src[(size_t)s * n + p.in_idx[j]];
      for (int o = 0; o < ch.nout; ++o)
        r[1 + ch.nin + o] = (uint64_t)(uintptr_t)dst[(size_t)s * n + p.out_idx[o0 + o]];
    }
    o0 += ch.nout;
  }
}

// Upload the rows of `launches` as one table and run them on `st`: pre() (an int code; what the
// call enqueues ahead of its kernels) once the table and the programs' uploads `up` are complete,
// then run(launch, its rows on the device, their count) per launch. The table is retired behind
// the launches. Without rows nothing happens (pre() is not called).
extern "C++" template <class Pre, class Run>
static int run_ptr_table(cec_codec* c, const std::vector<PtrLaunch>& launches, Uploads& up,
                         hipStream_t st, Pre pre, Run run) {
  size_t words = 0;
  for (const auto& l : launches) words += l.rows.size();
  if (!words) return CEC_OK;
  std::vector<uint64_t> host;
  host.reserve(words);
  for (const auto& l : launches) host.insert(host.end(), l.rows.begin(), l.rows.end());
  void* d = nullptr;
  const size_t bytes = words * sizeof(uint64_t);
  int rc = c->pool.alloc(bytes, &d);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(d, host.data(), bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the programs' uploads too
  if (e != hipSuccess) {
    c->pool.retire(d, bytes);
    return set_err(CEC_EHIP, std::string("table upload: ") + hipGetErrorString(e));
  }
  up.arena.reset();
  if ((rc = pre())) {
    c->pool.retire(d, bytes);
    return rc;
  }
  const uint64_t* tab = static_cast<const uint64_t*>(d);
  for (const auto& l : launches) {
    run(l, tab, (uint32_t)(l.rows.size() / l.rs));
    rc = check_launch();
    if (rc) break;
    tab += l.rows.size();
  }
  const int mrc = c->pool.mark(st);  // the table and the programs stay until these complete
  c->pool.retire(d, bytes);
  return rc ? rc : mrc;
}

// Behind the launches of call `what` (rc: their code, kept when set): clear the shard_len bytes at
// every address of `zeros`, the outputs whose product is of nothing.
static int clear_shards(int rc, const std::vector<uint8_t*>& zeros, size_t shard_len,
                        hipStream_t st, const char* what) {
  for (uint8_t* z : zeros) {
    if (rc) break;
    const hipError_t e = hipMemsetAsync(z, 0, shard_len, st);
    if (e != hipSuccess) rc = set_err(CEC_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  return rc;
}

// cec_reconstruct_ptrs, cec_encode_ptrs and, with `d_ok`, cec_verify_ptrs. There `dst` names
// expectations: the same programs and rows, run with PtrSink::compare, which reads what dst names
// and writes only d_ok (preset to 1 here, behind the validation). Their rows also hold the segment
// index, see kernels.h.
static int reconstruct_ptrs_impl(cec_codec* c, const uint8_t* const* src, uint8_t* const* dst,
                                 size_t nseg, size_t shard_len, hipStream_t st,
                                 uint8_t* d_ok = nullptr) {
  const int n = c->k + c->m, k = c->k;
  struct Group {
    ProgPtr prog;
    std::vector<uint32_t> segs;
  };
  std::unordered_map<std::string, size_t> gidx;
  std::vector<Group> groups;
  Uploads up{c->stream, c->arena};  // synchronised once, with the table's upload
  std::string key(2 * (size_t)n, '\0');
  uintptr_t bits = 0;  // OR of every address read or written: the alignment of the call
  for (size_t s = 0; s < nseg; ++s) {
    const uint8_t* const* sp = src + s * n;
    uint8_t* const* dp = dst + s * n;
    for (int i = 0; i < n; ++i) {
      if (d_ok && sp[i] && dp[i])
        return set_err(CEC_EINVAL, "a shard is both a source and an expectation");
      key[i] = sp[i] ? 1 : 0;
      key[n + i] = !sp[i] && dp[i] ? 1 : 0;
    }
    const size_t gi = group_of(gidx, key, groups.size());
    if (gi == groups.size()) {
      const uint8_t* f = reinterpret_cast<const uint8_t*>(key.data());
      ProgPtr p;
      if (int rc = get_decode(c, f, false, &p, &up.arena, f + n)) return rc;
      groups.push_back({p, {}});
    }
    Group& g = groups[gi];
    const Program& p = *g.prog;
    if (!p.nout) continue;  // nothing wanted: no row, no work
    for (int o = 0; o < p.nout; ++o) {
      const uint8_t* d = dp[p.out_idx[o]];
      bits |= (uintptr_t)d;
      if (d_ok) continue;  // a compare only reads: aliases are harmless
      for (int j = 0; j < k; ++j)
        if (d == sp[p.in_idx[j]])
          return set_err(CEC_EINVAL, "a destination is a survivor of its own segment");
    }
    for (int j = 0; j < k; ++j) bits |= (uintptr_t)sp[p.in_idx[j]];
    g.segs.push_back((uint32_t)s);
  }
  const bool vec_ok = (bits & 15) == 0;
  // launches: RS(2,1) rows for the compile-time kernel; otherwise one launch per (kernel, bucket)
  // over the rows of every pattern's chunk of that kind
  std::vector<PtrLaunch> launches;
  const bool ct21 = k == 2 && c->m == 1 && !c->force_generic;
  bool any_rows = false;
  for (const Group& g : groups) {
    const Program& p = *g.prog;
    if (!p.nout || g.segs.empty()) continue;
    any_rows = true;
    if (ct21) add_rs21_rows(c, launches, p, g.segs, src, dst, d_ok != nullptr);
    else add_rt_rows(c, launches, p, g.segs, src, dst, d_ok != nullptr);
  }
  auto preset_ok = [&]() -> int {
    if (!d_ok) return CEC_OK;
    const hipError_t e = hipMemsetAsync(d_ok, 1, nseg, st);
    return e == hipSuccess ? CEC_OK
                           : set_err(CEC_EHIP, std::string("verify: ") + hipGetErrorString(e));
  };
  int rc = CEC_OK;
  if (any_rows)
    rc = run_ptr_table(c, launches, up, st, preset_ok,
                       [&](const PtrLaunch& l, const uint64_t* tab, uint32_t nrows) {
                         launch_ptr_rows(l, d_ok ? cec::PtrSink::compare : cec::PtrSink::store,
                                         tab, nrows, shard_len, vec_ok, d_ok, st);
                       });
  else  // no segment has an expectation: every flag is 1
    rc = preset_ok();
  evict_decode(c);
  return rc;
}

// cec_reconstruct_partial_ptrs: the sibling of the above for partial rebuilds. A segment's program
// comes through get_partial (the decode rows of its pattern restricted to the held survivors,
// and to the wanted outputs), its rows go to the run-time kernels whatever the code, and with
// `accumulate` those are the accumulate forms. A segment with wanted outputs and no held survivor
// has no program: its outputs are cleared (or, with accumulate, left alone).
static int partial_ptrs_impl(cec_codec* c, const uint8_t* const* src, uint8_t* const* dst,
                             const uint8_t* present, size_t nseg, size_t shard_len,
                             bool accumulate, hipStream_t st) {
  const int n = c->k + c->m, k = c->k;
  struct Group {
    ProgPtr prog;  // null: no held survivor
    std::vector<uint32_t> segs;
  };
  std::unordered_map<std::string, size_t> gidx;
  std::vector<Group> groups;
  Uploads up{c->stream, c->arena};  // synchronised once, with the table's upload
  std::string key(3 * (size_t)n, '\0');  // present, held, wanted
  uintptr_t bits = 0;  // OR of every address read or written: the alignment of the call
  std::unordered_set<uintptr_t> seen;  // every wanted dst of the call
  std::vector<uint8_t*> zeros;         // wanted dst of segments without a held survivor
  for (size_t s = 0; s < nseg; ++s) {
    const uint8_t* const* sp = src + s * n;
    uint8_t* const* dp = dst + s * n;
    const uint8_t* pr = present + s * n;
    int np = 0;
    bool wanted = false;
    for (int i = 0; i < n; ++i) {
      if (sp[i] && !pr[i]) return set_err(CEC_EINVAL, "a shard flagged absent is held");
      key[i] = pr[i] ? 1 : 0;
      key[n + i] = sp[i] ? 1 : 0;
      key[2 * n + i] = !pr[i] && dp[i] ? 1 : 0;
      np += key[i];
      wanted |= key[2 * n + i] != 0;
    }
    if (!wanted) continue;  // nothing wanted: no row, no work, shards not counted
    if (np < k) return set_err(CEC_ETOOFEW, "fewer than k shards present");
    const size_t gi = group_of(gidx, key, groups.size());
    if (gi == groups.size()) {
      const uint8_t* f = reinterpret_cast<const uint8_t*>(key.data());
      uint8_t rd[cec::kMaxShards];
      if (!cec::survivor_set(k, c->m, f, rd))
        return set_err(CEC_ETOOFEW, "fewer than k shards present");
      bool held = false;
      for (int i = 0; i < n; ++i) held |= rd[i] && f[n + i];
      ProgPtr p;
      if (held)
        if (int rc = get_partial(c, f, f + n, false, &p, &up.arena, nullptr, f + 2 * n)) return rc;
      groups.push_back({p, {}});
    }
    Group& g = groups[gi];
    for (int i = 0; i < n; ++i) {
      if (!key[2 * n + i]) continue;
      if (!seen.insert((uintptr_t)dp[i]).second)
        return set_err(CEC_EINVAL, "a destination is named twice");
      if (!g.prog && !accumulate) zeros.push_back(dp[i]);
    }
    if (!g.prog) continue;
    const Program& p = *g.prog;
    const int nin = p.chunks[0].nin;  // the held survivors, in cec_survivors order
    for (int o = 0; o < p.nout; ++o) {
      const uint8_t* d = dp[p.out_idx[o]];
      bits |= (uintptr_t)d;
      for (int j = 0; j < nin; ++j)
        if (d == sp[p.in_idx[j]])
          return set_err(CEC_EINVAL, "a destination is a held survivor of its own segment");
    }
    for (int j = 0; j < nin; ++j) bits |= (uintptr_t)sp[p.in_idx[j]];
    g.segs.push_back((uint32_t)s);
  }
  const bool vec_ok = (bits & 15) == 0;
  std::vector<PtrLaunch> launches;
  for (const Group& g : groups)
    if (g.prog && !g.segs.empty()) add_rt_rows(c, launches, *g.prog, g.segs, src, dst, false);
  const cec::PtrSink sink = accumulate ? cec::PtrSink::accumulate : cec::PtrSink::store;
  int rc = run_ptr_table(
      c, launches, up, st, [] { return (int)CEC_OK; },
      [&](const PtrLaunch& l, const uint64_t* tab, uint32_t nrows) {
        launch_ptr_rows(l, sink, tab, nrows, shard_len, vec_ok, nullptr, st);
      });
  // zero is the neutral element of the exchange's sum
  rc = clear_shards(rc, zeros, shard_len, st, "partial");
  evict_decode(c);
  return rc;
}

int cec_reconstruct_ptrs(cec_codec* c, const uint8_t* const* src, uint8_t* const* dst,
                         size_t nseg, size_t shard_len, void* hip_stream) {
  if (!c || (nseg && (!src || !dst))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  return reconstruct_ptrs_impl(c, src, dst, nseg, shard_len, pick_stream(c, hip_stream));
}

int cec_encode_ptrs(cec_codec* c, const uint8_t* const* d_data_ptrs, uint8_t* const* d_parity_ptrs,
                    size_t nseg, size_t shard_len, void* hip_stream) {
  if (!c || (nseg && (!d_data_ptrs || !d_parity_ptrs))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  const int n = c->k + c->m;
  std::vector<const uint8_t*> src(nseg * n, nullptr);
  std::vector<uint8_t*> dst(nseg * n, nullptr);
  for (size_t s = 0; s < nseg; ++s) {
    for (int i = 0; i < c->k; ++i)
      if (!(src[s * n + i] = d_data_ptrs[s * c->k + i])) return set_err(CEC_EINVAL, "null shard");
    for (int o = 0; o < c->m; ++o)
      if (!(dst[s * n + c->k + o] = d_parity_ptrs[s * c->m + o]))
        return set_err(CEC_EINVAL, "null shard");
  }
  CEC_HIP_TRY(hipSetDevice(c->device));
  return reconstruct_ptrs_impl(c, src.data(), dst.data(), nseg, shard_len,
                               pick_stream(c, hip_stream));
}

int cec_verify_ptrs(cec_codec* c, const uint8_t* const* src, const uint8_t* const* expect,
                    size_t nseg, size_t shard_len, uint8_t* d_ok, void* hip_stream) {
  if (!c || (nseg && (!src || !expect || !d_ok))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  // the expectations sit where a rebuild's destinations do; the compare kernels only read them
  return reconstruct_ptrs_impl(c, src, const_cast<uint8_t* const*>(expect), nseg, shard_len,
                               pick_stream(c, hip_stream), d_ok);
}

int cec_reconstruct_partial_ptrs(cec_codec* c, const uint8_t* const* src, uint8_t* const* dst,
                                 const uint8_t* present, size_t nseg, size_t shard_len,
                                 int accumulate, void* hip_stream) {
  if (!c || (nseg && (!src || !dst || !present))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  return partial_ptrs_impl(c, src, dst, present, nseg, shard_len, accumulate != 0,
                           pick_stream(c, hip_stream));
}

int cec_xor_ptrs(cec_codec* c, uint8_t* const* dst, const uint8_t* const* src, size_t nrows,
                 size_t nsrc, size_t len, void* hip_stream) {
  if (!c) return set_err(CEC_EINVAL, "null");
  if (len == 0 || nrows == 0 || nsrc == 0) return CEC_OK;
  if (!dst || !src) return set_err(CEC_EINVAL, "null");
  if (nrows > 0x7fffffffull || nsrc > 0x7ffffffeull)
    return set_err(CEC_EINVAL, "too many rows or sources");
  if ((len + 255) / 256 > 0x7fffffffull) return set_err(CEC_EINVAL, "len too large (> 512 GiB)");
  // every address is checked, also those of rows that get no work: the arrays are then wrong
  // whichever rows run
  std::unordered_set<uintptr_t> dsts;
  for (size_t r = 0; r < nrows; ++r)
    if (dst[r] && !dsts.insert((uintptr_t)dst[r]).second)
      return set_err(CEC_EINVAL, "a destination is named twice");
  for (size_t i = 0; i < nrows * nsrc; ++i)
    if (src[i] && dsts.count((uintptr_t)src[i]))
      return set_err(CEC_EINVAL, "a source is a destination of the call");
  std::vector<PtrLaunch> launches(1);
  PtrLaunch& l = launches[0];
  // rows {dst, nsrc sources}, NULL sources kept as 0
  l = {PtrKind::xor_rows, 0, (uint32_t)(nsrc + 1), {}};
  uintptr_t bits = 0;
  for (size_t r = 0; r < nrows; ++r) {
    if (!dst[r]) continue;
    const uint8_t* const* sp = src + r * nsrc;
    if (std::all_of(sp, sp + nsrc, [](const uint8_t* p) { return !p; })) continue;
    l.rows.push_back((uint64_t)(uintptr_t)dst[r]);
    bits |= (uintptr_t)dst[r];
    for (size_t j = 0; j < nsrc; ++j) {
      l.rows.push_back((uint64_t)(uintptr_t)sp[j]);
      bits |= (uintptr_t)sp[j];
    }
  }
  if (l.rows.empty()) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, hip_stream);
  const bool vec_ok = (bits & 15) == 0;
  Uploads up{c->stream, c->arena};
  return run_ptr_table(c, launches, up, st, [] { return (int)CEC_OK; },
                       [&](const PtrLaunch& x, const uint64_t* tab, uint32_t n) {
                         cec::launch_xor_rows(tab, n, (uint32_t)nsrc, len, vec_ok, st);
                       });
}

static_assert(CEC_FLAG_CLEAN == cec::kFlagClean && CEC_FLAG_REBUILT == cec::kFlagRebuilt &&
                  CEC_FLAG_MANY == cec::kFlagMany && CEC_FLAG_LOST == cec::kFlagLost,
              "the planner kernels write the header's codes");

int cec_flag_status(int k, int m, const uint8_t* held, const uint8_t* flags, int* status,
                    int* lost) {
  if (!held || !flags || !status) return set_err(CEC_EINVAL, "null");
  if (k < 1 || m < 1 || k + m > cec::kMaxShards)
    return set_err(CEC_EINVAL, "need k >= 1, m >= 1, k + m <= 256");
  int bad = 0, good = 0, first = -1;
  for (int i = 0; i < k + m; ++i) {
    if (!held[i]) continue;
    if (flags[i]) {
      ++good;
    } else if (bad++ == 0) {
      first = i;
    }
  }
  *status = bad == 0 ? CEC_FLAG_CLEAN
            : good < k ? CEC_FLAG_LOST
            : bad == 1 ? CEC_FLAG_REBUILT
                       : CEC_FLAG_MANY;
  if (lost) *lost = *status == CEC_FLAG_REBUILT ? first : -1;
  return CEC_OK;
}

// The calls that decide on the GPU keep their tables in one pool block. `words` of `host` go to
// its front on c->stream, which is synchronised: the one host wait of such a call, never on `st`.
static int upload_table(cec_codec* c, void* d, const uint64_t* host, size_t words) {
  hipError_t e = hipMemcpyAsync(d, host, words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) return CEC_OK;
  return set_err(CEC_EHIP, std::string("table upload: ") + hipGetErrorString(e));
}
// Behind the call's launches: the block stays until what is queued on `st` completes.
static int retire_behind(cec_codec* c, void* d, size_t bytes, hipStream_t st, int rc) {
  const int mrc = c->pool.mark(st);
  c->pool.retire(d, bytes);
  return rc ? rc : mrc;
}

// cec_repair_flagged_ptrs: which shard of a segment is rebuilt is decided on the device, from
// flags that may not exist yet when this returns, so the host prepares every answer. Segments are
// grouped by held set; for a group that holds more than k shards, every held shard j gets the
// program cec_reconstruct_ptrs would use for (held \ {j}, required {j}). The planner kernel
// (kernels.h FlagPlan) picks per segment and writes the working table; the product launches
// behind it cover every segment and leave at once where the planner wrote an idle row. Nothing
// here waits for `st` or copies from the device. RS(2,1)'s compile-time rows need no program.
static int repair_flagged_impl(cec_codec* c, uint8_t* const* shards, const uint8_t* d_flags,
                               size_t nseg, size_t shard_len, uint8_t* d_status, hipStream_t st) {
  const int n = c->k + c->m, k = c->k;
  const bool ct21 = k == 2 && c->m == 1 && !c->force_generic;
  const uint32_t rs = ct21 ? 4u : (uint32_t)k + 2;
  // any shard may become a destination: the same address twice is two rows that may race
  std::unordered_set<uintptr_t> seen;
  uintptr_t bits = 0;  // OR of every held address: the alignment of the call
  for (size_t i = 0; i < nseg * n; ++i) {
    if (!shards[i]) continue;
    if (!seen.insert((uintptr_t)shards[i]).second)
      return set_err(CEC_EINVAL, "a shard address is named twice");
    bits |= (uintptr_t)shards[i];
  }
  const bool vec_ok = (bits & 15) == 0;
  struct Group {
    std::vector<ProgPtr> progs;  // by lost shard; null where the held set cannot lose that one
  };
  std::unordered_map<std::string, size_t> gidx;
  std::vector<Group> groups;
  Uploads up{c->stream, c->arena};  // synchronised once, with the table's upload
  std::string key((size_t)n, '\0');
  // the upload: [nseg][n + 1] addresses and group, [group][n] chunks, [group][n][k] survivors
  std::vector<uint64_t> host(nseg * (n + 1), 0);
  bool any_prog = false;
  for (size_t s = 0; s < nseg; ++s) {
    int nheld = 0;
    for (int i = 0; i < n; ++i) {
      host[s * (n + 1) + i] = (uint64_t)(uintptr_t)shards[s * n + i];
      key[i] = shards[s * n + i] ? 1 : 0;
      nheld += key[i];
    }
    if (ct21) continue;  // one group, no programs
    const size_t gi = group_of(gidx, key, groups.size());
    host[s * (n + 1) + n] = gi;
    if (gi < groups.size()) continue;
    groups.push_back({std::vector<ProgPtr>(n)});
    if (nheld <= k) continue;  // one bad shard leaves fewer than k: nothing can be rebuilt
    uint8_t present[cec::kMaxShards], required[cec::kMaxShards] = {};
    for (int i = 0; i < n; ++i) present[i] = (uint8_t)key[i];
    for (int j = 0; j < n; ++j) {
      if (!key[j]) continue;
      present[j] = 0;
      required[j] = 1;
      ProgPtr p;
      const int rc = get_decode(c, present, false, &p, &up.arena, required);
      present[j] = 1;
      required[j] = 0;
      if (rc) return rc;
      if (p->nout != 1 || p->chunks.size() != 1 || p->chunks[0].nob != 1 ||
          p->chunks[0].nin != k || p->out_idx[0] != j)
        return set_err(CEC_EINVAL, "a one-shard rebuild is not one chunk of one output");
      groups.back().progs[j] = std::move(p);
      any_prog = true;
    }
  }
  const size_t ng = groups.size();
  const size_t chunks_at = host.size(), surv_at = chunks_at + ng * n;
  const size_t in_words = surv_at + (ng * n * k + 7) / 8;
  host.resize(in_words, 0);
  uint8_t* surv = reinterpret_cast<uint8_t*>(host.data() + surv_at);
  for (size_t g = 0; g < ng; ++g)
    for (int j = 0; j < n; ++j) {
      const ProgPtr& p = groups[g].progs[j];
      if (!p) continue;
      host[chunks_at + g * n + j] = (uint64_t)(uintptr_t)p->chunks[0].dev;
      std::memcpy(surv + (g * n + j) * k, p->in_idx, k);
    }
  void* d = nullptr;
  const size_t bytes = (in_words + nseg * rs) * sizeof(uint64_t);
  int rc = c->pool.alloc(bytes, &d);
  if (rc) return rc;
  rc = upload_table(c, d, host.data(), in_words);  // the programs' uploads too
  up.arena.reset();
  if (rc) {
    c->pool.retire(d, bytes);
    return rc;
  }
  uint64_t* dw = static_cast<uint64_t*>(d);
  cec::FlagPlan fp{};
  fp.segs = dw;
  fp.chunks = dw + chunks_at;
  fp.surv = reinterpret_cast<const uint8_t*>(dw + surv_at);
  fp.flags = d_flags;
  fp.status = d_status;
  fp.rows = dw + in_words;
  fp.nseg = (uint32_t)nseg;
  fp.n = n;
  fp.k = k;
  cec::launch_flag_plan(fp, ct21, st);
  rc = check_launch();
  if (!rc && ct21) {
    cec::launch_ptrs_rs21(cec::PtrSink::store, fp.rows, fp.nseg, shard_len, vec_ok, nullptr, st);
    rc = check_launch();
  } else if (!rc && any_prog) {  // without a program every row is idle
    cec::launch_ptrs_rt_flag(cec::rt_takes_rtb(c->opts, 1, k), fp.rows, fp.nseg, rs, 1, shard_len,
                             vec_ok, st);
    rc = check_launch();
  }
  rc = retire_behind(c, d, bytes, st, rc);  // the table and the programs
  evict_decode(c);  // `groups` holds the call's programs to the end
  return rc;
}

int cec_repair_flagged_ptrs(cec_codec* c, uint8_t* const* shards, const uint8_t* d_flags,
                            size_t nseg, size_t shard_len, uint8_t* d_status, void* hip_stream) {
  if (!c || (nseg && (!shards || !d_flags || !d_status))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  return repair_flagged_impl(c, shards, d_flags, nseg, shard_len, d_status,
                             pick_stream(c, hip_stream));
}

static_assert(CEC_FLAG_MULTI_MAX == cec::kFlagMultiMax, "the planner kernel's bound");
static_assert(CEC_FLAG_CLEAN == cec::kFsClean && CEC_FLAG_REBUILT == cec::kFsRebuilt &&
                  CEC_FLAG_MANY == cec::kFsMany && CEC_FLAG_LOST == cec::kFsLost,
              "flag_solve.h states the rule in the header's codes");

static int check_flag_multi(int k, int m, int max_bad) {
  if (k < 1 || m < 1 || k + m > cec::kMaxShards)
    return set_err(CEC_EINVAL, "need k >= 1, m >= 1, k + m <= 256");
  if (max_bad < 1 || max_bad > CEC_FLAG_MULTI_MAX)
    return set_err(CEC_EINVAL, "max_bad must be 1..CEC_FLAG_MULTI_MAX");
  return CEC_OK;
}

int cec_flag_solve(int k, int m, const uint8_t* held, const uint8_t* flags, int max_bad,
                   int* status, int* nout, uint8_t* out_idx, uint8_t* in_idx, uint8_t* rows) {
  if (!held || !flags || !status || !nout) return set_err(CEC_EINVAL, "null");
  if (int rc = check_flag_multi(k, m, max_bad)) return rc;
  uint32_t st = 0, e = 0;
  cec::fs_plan_segment((uint32_t)k, (uint32_t)(k + m), held, flags, (uint32_t)max_bad, &st, &e,
                       out_idx, in_idx, rows, nullptr);
  *status = (int)st;
  *nout = (int)e;
  return CEC_OK;
}

int cec_flag_status_multi(int k, int m, const uint8_t* held, const uint8_t* flags, int max_bad,
                          int* status, int* nlost, uint8_t* lost) {
  if (!nlost) return set_err(CEC_EINVAL, "null");
  return cec_flag_solve(k, m, held, flags, max_bad, status, nlost, lost, nullptr, nullptr);
}

// What cec_repair_flagged_multi_ptrs and cec_read_flagged_ptrs do once the caller has scanned its
// addresses into `host` (the [nseg][n] shard addresses first) and filled what it knows of `fp`.
// One pool block: the upload, `mid_words` words of the caller's (the read's copy rows), then the
// product rows: bucket b's table [nseg][k + 1 + b] for b <= widest, or with `ct21` RS(2,1)'s
// [nseg][4]. The segments' chunks are scratch on `st`. plan(fp, mid) launches the planner, and
// what else comes before the products, over the completed plan and returns a status; one product
// launch per table follows it. Nothing here waits for `st` or copies from the device, and the
// decode cache is not touched.
extern "C++" template <class Plan>
static int run_flag_plan(cec_codec* c, const std::vector<uint64_t>& host, size_t mid_words,
                         bool ct21, int widest, cec::FlagPlanMulti fp, size_t shard_len,
                         bool vec_ok, hipStream_t st, Plan plan) {
  const uint32_t k = (uint32_t)fp.k;
  const size_t nseg = fp.nseg;
  const int tables = ct21 ? 1 : widest;  // < 1: every row of the call is idle
  size_t words = host.size() + mid_words, rows_at[CEC_FLAG_MULTI_MAX] = {};
  for (int b = 1; b <= tables; ++b) {
    rows_at[b - 1] = words;
    words += nseg * (ct21 ? cec::kRp21RowWords : cec::fs_row_words(k, (uint32_t)b));
  }
  const size_t bytes = words * sizeof(uint64_t);
  void* d = nullptr;
  int rc = c->pool.alloc(bytes, &d);
  if (rc) return rc;
  // the segments' chunks: written and read on `st` only, so a large block is stream-ordered
  const size_t chunk_words = ct21 || widest < 1 ? 0 : cec::fs_chunk_words(k, (uint32_t)widest);
  Scratch progs;
  if (chunk_words) rc = scratch_alloc(c, nseg * chunk_words * sizeof(uint32_t), st, &progs);
  if (!rc) rc = upload_table(c, d, host.data(), host.size());
  if (rc) {
    c->pool.retire(d, bytes);
    scratch_release(c, progs, st);
    return rc;
  }
  uint64_t* dw = static_cast<uint64_t*>(d);
  fp.segs = dw;
  for (int b = 1; b <= tables; ++b) fp.rows[b - 1] = dw + rows_at[b - 1];
  fp.chunks = static_cast<uint32_t*>(progs.p);
  fp.chunk_words = (uint32_t)chunk_words;
  rc = plan(fp, dw + host.size());
  if (!rc && ct21) {
    cec::launch_ptrs_rs21(cec::PtrSink::store, fp.rows[0], fp.nseg, shard_len, vec_ok, nullptr, st);
    rc = check_launch();
  }
  for (int b = 1; !ct21 && b <= widest && !rc; ++b) {
    cec::launch_ptrs_rt_flag(cec::rt_takes_rtb(c->opts, b, (int)k), fp.rows[b - 1], fp.nseg,
                             cec::fs_row_words(k, (uint32_t)b), b, shard_len, vec_ok, st);
    rc = check_launch();
  }
  rc = retire_behind(c, d, bytes, st, rc);  // the tables; the chunks stay as long
  scratch_release(c, progs, st);
  return rc;
}

// cec_repair_flagged_multi_ptrs: nothing about a segment is known on the host but what it holds,
// so the host uploads the addresses and nothing else; the planner kernel (kernels.h
// FlagPlanMulti) solves every rebuilt segment's rows and writes its program chunk and its table
// row. One table per bucket b <= max_bad that some held set of the call can fill (k + b shards
// held), one product launch over all of it behind the planner (run_flag_plan).
static int repair_flagged_multi_impl(cec_codec* c, uint8_t* const* shards, const uint8_t* d_flags,
                                     size_t nseg, size_t shard_len, int max_bad,
                                     uint8_t* d_status, hipStream_t st) {
  const int n = c->k + c->m, k = c->k;
  std::unordered_set<uintptr_t> seen;
  uintptr_t bits = 0;  // OR of every held address: the alignment of the call
  std::vector<uint64_t> host(nseg * n, 0);
  int most = 0;  // the largest held set
  for (size_t s = 0; s < nseg; ++s) {
    int nheld = 0;
    for (int i = 0; i < n; ++i) {
      uint8_t* const a = shards[s * n + i];
      if (!a) continue;
      if (!seen.insert((uintptr_t)a).second)
        return set_err(CEC_EINVAL, "a shard address is named twice");
      bits |= (uintptr_t)a;
      host[s * n + i] = (uint64_t)(uintptr_t)a;
      ++nheld;
    }
    most = std::max(most, nheld);
  }
  cec::FlagPlanMulti fp{};
  fp.flags = d_flags;
  fp.status = d_status;
  fp.nseg = (uint32_t)nseg;
  fp.n = n;
  fp.k = k;
  fp.max_bad = max_bad;
  return run_flag_plan(c, host, 0, false, std::min({max_bad, c->m, most - k}), fp, shard_len,
                       (bits & 15) == 0, st, [&](const cec::FlagPlanMulti& p, uint64_t*) {
                         cec::launch_flag_plan_multi(p, st);
                         return check_launch();
                       });
}

int cec_repair_flagged_multi_ptrs(cec_codec* c, uint8_t* const* shards, const uint8_t* d_flags,
                                  size_t nseg, size_t shard_len, int max_bad, uint8_t* d_status,
                                  void* hip_stream) {
  if (!c || (nseg && (!shards || !d_flags || !d_status))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_flag_multi(c->k, c->m, max_bad)) return rc;
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  // one bad shard per segment at the most: the single-failure call, its planners and products
  if (c->m == 1 || max_bad == 1)
    return repair_flagged_impl(c, shards, d_flags, nseg, shard_len, d_status,
                               pick_stream(c, hip_stream));
  return repair_flagged_multi_impl(c, shards, d_flags, nseg, shard_len, max_bad, d_status,
                                   pick_stream(c, hip_stream));
}

// ---- a degraded read decided from flags (read_plan.h) -----------------------------------------

static int check_read_args(int k, int m, const uint8_t* held, const uint8_t* flags,
                           const uint8_t* wanted, int max_bad) {
  if (!held || !flags || !wanted) return set_err(CEC_EINVAL, "null");
  return check_flag_multi(k, m, max_bad);
}

int cec_read_solve(int k, int m, const uint8_t* held, const uint8_t* flags, const uint8_t* wanted,
                   int max_bad, int* status, int* nout, uint8_t* out_idx, uint8_t* in_idx,
                   uint8_t* rows, uint8_t* copy_idx, int* ncopy) {
  if (!status || !nout || !ncopy) return set_err(CEC_EINVAL, "null");
  if (int rc = check_read_args(k, m, held, flags, wanted, max_bad)) return rc;
  uint32_t st = 0, e = 0, nc = 0;
  cec::rp_plan_segment((uint32_t)k, (uint32_t)(k + m), held, flags, wanted, (uint32_t)max_bad, &st,
                       &e, out_idx, in_idx, rows, nullptr, copy_idx, &nc, nullptr);
  *status = (int)st;
  *nout = (int)e;
  *ncopy = (int)nc;
  return CEC_OK;
}

int cec_read_status(int k, int m, const uint8_t* held, const uint8_t* flags, const uint8_t* wanted,
                    int max_bad, int* status, int* nmiss, uint8_t* miss) {
  if (!nmiss) return set_err(CEC_EINVAL, "null");
  int ncopy = 0;
  return cec_read_solve(k, m, held, flags, wanted, max_bad, status, nmiss, miss, nullptr, nullptr,
                        nullptr, &ncopy);
}

// cec_read_flagged_ptrs: cec_repair_flagged_multi_ptrs aimed at a destination. The host uploads
// the shard addresses and the destinations and nothing else; the planner (kernels.h ReadPlan)
// applies the rule, writes the copy rows of every segment and, for a rebuilt one, its program
// chunk and its product row; the gated copy and one product launch per bucket follow it on `st`
// (run_flag_plan). RS(2,1) takes k_ptr21's closed forms and needs no chunk.
static int read_flagged_impl(cec_codec* c, const uint8_t* const* shards, const uint8_t* d_flags,
                             uint8_t* const* dst, size_t nseg, size_t shard_len, int max_bad,
                             uint8_t* d_status, hipStream_t st) {
  const int n = c->k + c->m, k = c->k;
  const bool ct21 = k == 2 && c->m == 1 && !c->force_generic;
  if (nseg * (size_t)k > 0xffffffffull) return set_err(CEC_EINVAL, "too many copy rows");
  // the upload: [nseg][n] shard addresses, then [nseg][k] destinations
  const size_t dst_at = nseg * n;
  std::vector<uint64_t> host(dst_at + nseg * k, 0);
  std::unordered_set<uintptr_t> held, outs;
  uintptr_t bits = 0;  // OR of every held address and every destination: the call's alignment
  int most = 0;        // the most shards any segment wants
  for (size_t i = 0; i < nseg * n; ++i) {
    if (!shards[i]) continue;
    held.insert((uintptr_t)shards[i]);
    bits |= (uintptr_t)shards[i];
    host[i] = (uint64_t)(uintptr_t)shards[i];
  }
  for (size_t s = 0; s < nseg; ++s) {
    int want = 0;
    for (int j = 0; j < k; ++j) {
      uint8_t* const a = dst[s * k + j];
      if (!a) continue;
      if (!outs.insert((uintptr_t)a).second)
        return set_err(CEC_EINVAL, "a destination address is named twice");
      if (held.count((uintptr_t)a))
        return set_err(CEC_EINVAL, "a destination is a shard of the call (the repair heals in place)");
      bits |= (uintptr_t)a;
      host[dst_at + s * k + j] = (uint64_t)(uintptr_t)a;
      ++want;
    }
    most = std::max(most, want);
  }
  const bool vec_ok = (bits & 15) == 0;
  cec::ReadPlan rp{};
  rp.flags = d_flags;
  rp.status = d_status;
  rp.nseg = (uint32_t)nseg;
  rp.n = n;
  rp.k = k;
  rp.max_bad = max_bad;
  // a segment rebuilds its missing wanted data shards: at most max_bad, m (k good ones remain) and
  // what it wants. < 1: nothing is wanted anywhere, every row of the call is idle. The copy rows
  // [nseg][k][2] lie between the upload and the product rows
  return run_flag_plan(c, host, nseg * (size_t)k * cec::kRpCopyWords, ct21,
                       std::min({max_bad, c->m, most}), rp, shard_len, vec_ok, st,
                       [&](cec::ReadPlan& p, uint64_t* copy_rows) {
                         p.dst = p.segs + dst_at;
                         p.copy = copy_rows;
                         cec::launch_read_plan(p, ct21, st);
                         if (int rc = check_launch()) return rc;
                         cec::launch_read_copy(p.copy, (uint64_t)nseg * k, shard_len, vec_ok, st);
                         return check_launch();
                       });
}

int cec_read_flagged_ptrs(cec_codec* c, const uint8_t* const* shards, const uint8_t* d_flags,
                          uint8_t* const* dst, size_t nseg, size_t shard_len, int max_bad,
                          uint8_t* d_status, void* hip_stream) {
  if (!c || (nseg && (!shards || !d_flags || !dst || !d_status)))
    return set_err(CEC_EINVAL, "null");
  if (int rc = check_flag_multi(c->k, c->m, max_bad)) return rc;
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  return read_flagged_impl(c, shards, d_flags, dst, nseg, shard_len, max_bad, d_status,
                           pick_stream(c, hip_stream));
}

// ---- the corrupt shard from parity alone (locate_rule.h) ---------------------------------------

static_assert(CEC_LOCATE_SYN_MAX == cec::kLocateSynMax, "one syndrome product per bucket");
static_assert(CEC_LOCATE_CLEAN == cec::kLocClean && CEC_LOCATE_FOUND == cec::kLocFound &&
                  CEC_LOCATE_AMBIGUOUS == cec::kLocAmbiguous &&
                  CEC_LOCATE_UNCHECKED == cec::kLocUnchecked,
              "locate_rule.h states the rule in the header's codes");

static int check_locate(int k, int m, int nsyn) {
  if (k < 1 || m < 1 || k + m > cec::kMaxShards)
    return set_err(CEC_EINVAL, "need k >= 1, m >= 1, k + m <= 256");
  if (nsyn < 1 || nsyn > CEC_LOCATE_SYN_MAX)
    return set_err(CEC_EINVAL, "nsyn must be 1..CEC_LOCATE_SYN_MAX");
  return CEC_OK;
}

int cec_locate_rows(int k, int m, const uint8_t* held, int nsyn, int* r, uint8_t* rows) {
  if (!held || !r || !rows) return set_err(CEC_EINVAL, "null");
  if (int rc = check_locate(k, m, nsyn)) return rc;
  const uint32_t n = (uint32_t)(k + m);
  uint8_t H[cec::kMaxShards];
  uint32_t h = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (held[i]) H[h++] = (uint8_t)i;
  const uint32_t rr = cec::loc_r(h, (uint32_t)k, (uint32_t)nsyn);
  std::memset(rows, 0, (size_t)CEC_LOCATE_SYN_MAX * n);
  for (uint32_t t = 0; t < h && rr; ++t) {
    const uint32_t col = cec::loc_column(H, h, t);
    for (uint32_t a = 0; a < rr; ++a) rows[(size_t)a * n + H[t]] = (uint8_t)(col >> (8 * a));
  }
  *r = (int)rr;
  return CEC_OK;
}

int cec_locate_host(int k, int m, const uint8_t* const* shards, size_t shard_len, int nsyn,
                    int* status, int* found) {
  if (!shards || !status || !found) return set_err(CEC_EINVAL, "null");
  if (int rc = check_locate(k, m, nsyn)) return rc;
  uint32_t st = 0;
  cec::loc_segment_host((uint32_t)k, (uint32_t)(k + m), shards, shard_len, (uint32_t)nsyn, &st,
                        found);
  *status = (int)st;
  return CEC_OK;
}

// cec_locate_ptrs: the held sets are the NULL pattern, so the host knows them all. One pool block:
// the upload ([nseg][most + 2] rows {chunk, held addresses in index order, ..., set}, the sets'
// planner tables, the sets' program chunks), then what the kernels keep between them (witness,
// candidate, dirty, dirty2 per segment), preset on `st`. One grid of the syndrome product per
// value of r in the call, the planner, the confirm grids, the finish. Nothing here waits for `st`
// or copies from the device, and the decode cache is not touched.
//
// cec_locate_multi_ptrs with max_bad = 2 (`pair`) takes the same rows and chunks, the planner
// tables with four coefficient rows, and two more arrays (the second witness, dirtyU): locate
// pass, first solve, T confirm, second solve, U confirm, finish. Without `pair` the launches are
// cec_locate_ptrs' own, and d_nbad, where given, is derived from the status they wrote.
static int locate_impl(cec_codec* c, const uint8_t* const* shards, size_t nseg, size_t shard_len,
                       int nsyn, bool pair, uint8_t* d_flags, uint8_t* d_status, uint8_t* d_nbad,
                       hipStream_t st) {
  const uint32_t n = (uint32_t)(c->k + c->m), k = (uint32_t)c->k;
  struct Set {
    std::string key;
    uint32_t h, r;
    size_t chunk_at;  // word offset of its chunk in the block (r >= 1)
  };
  std::unordered_map<std::string, size_t> gidx;
  std::vector<Set> sets;
  std::vector<uint32_t> set_of(nseg);
  std::string key((size_t)n, '\0');
  uintptr_t bits = 0;  // OR of every held address: the alignment of the call
  uint32_t most = 0;
  bool has_r[CEC_LOCATE_SYN_MAX + 1] = {};
  for (size_t s = 0; s < nseg; ++s) {
    uint32_t h = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint8_t* const a = shards[s * n + i];
      key[i] = a ? 1 : 0;
      h += a ? 1 : 0;
      bits |= (uintptr_t)a;
    }
    const size_t gi = group_of(gidx, key, sets.size());
    set_of[s] = (uint32_t)gi;
    if (gi < sets.size()) continue;
    const uint32_t r = cec::loc_r(h, k, (uint32_t)nsyn);
    sets.push_back({key, h, r, 0});
    most = std::max(most, h);
    has_r[r] = true;
  }
  const bool vec_ok = (bits & 15) == 0;
  const uint32_t rs = most + 2, set_bytes = pair ? cec::loc2_set_bytes(n) : cec::loc_set_bytes(n);
  const size_t sets_at = nseg * rs;
  size_t in_words = sets_at + sets.size() * (set_bytes / 8);
  for (Set& g : sets) {
    if (!g.r) continue;
    g.chunk_at = in_words;
    in_words += (cec::fs_chunk_words(g.h, g.r) + 1) / 2;
  }
  // witness (and the second one of the pair rule), candidate, then the dirty bytes
  const size_t wit_at = in_words, cand_at = wit_at + (pair ? 2 : 1) * nseg;
  const size_t dirty_at = cand_at + (nseg + 1) / 2, ndirty = (pair ? 3 : 2) * nseg;
  const size_t words = dirty_at + (ndirty + 7) / 8;
  const size_t bytes = words * sizeof(uint64_t);
  void* d = nullptr;
  int rc = c->pool.alloc(bytes, &d);
  if (rc) return rc;
  uint64_t* dw = static_cast<uint64_t*>(d);
  std::vector<uint64_t> host(in_words, 0);
  for (size_t g = 0; g < sets.size(); ++g) {
    const Set& set = sets[g];
    (pair ? cec::loc2_put_set : cec::loc_put_set)(
        reinterpret_cast<uint8_t*>(host.data() + sets_at) + g * set_bytes,
        reinterpret_cast<const uint8_t*>(set.key.data()), n, set.r);
    if (!set.r) continue;
    uint8_t H[cec::kMaxShards];
    uint32_t h = 0;
    for (uint32_t i = 0; i < n; ++i)
      if (set.key[i]) H[h++] = (uint8_t)i;
    cec::loc_put_chunk(reinterpret_cast<uint32_t*>(host.data() + set.chunk_at), H, h, set.r);
  }
  for (size_t s = 0; s < nseg; ++s) {
    const Set& set = sets[set_of[s]];
    uint64_t* row = host.data() + s * rs;
    row[rs - 1] = set_of[s];
    if (!set.r) continue;  // unchecked: no chunk and no address goes to the device
    row[0] = (uint64_t)(uintptr_t)(dw + set.chunk_at);
    uint32_t t = 0;
    for (uint32_t i = 0; i < n; ++i)
      if (shards[s * n + i]) row[1 + t++] = (uint64_t)(uintptr_t)shards[s * n + i];
  }
  rc = upload_table(c, d, host.data(), in_words);
  if (rc) {
    c->pool.retire(d, bytes);
    return rc;
  }
  if (pair) {
    cec::PairPlan pp{};
    pp.rows = dw;
    pp.sets = reinterpret_cast<const uint8_t*>(dw + sets_at);
    pp.witness = dw + wit_at;
    pp.witness2 = pp.witness + nseg;
    pp.cand = reinterpret_cast<uint32_t*>(dw + cand_at);
    pp.dirty = reinterpret_cast<uint8_t*>(dw + dirty_at);
    pp.dirtyT = pp.dirty + nseg;
    pp.dirtyU = pp.dirtyT + nseg;
    pp.flags = d_flags;
    pp.status = d_status;
    pp.nbad = d_nbad;
    pp.rs = rs;
    pp.set_bytes = set_bytes;
    pp.nseg = (uint32_t)nseg;
    pp.n = (int)n;
    pp.k = (int)k;
    pp.max_bad = CEC_LOCATE_BAD_MAX;
    hipError_t e = hipMemsetAsync(pp.witness, 0xFF, 2 * nseg * sizeof(uint64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(pp.dirty, 0, ndirty, st);
    if (e != hipSuccess)
      rc = set_err(CEC_EHIP, std::string("locate preset: ") + hipGetErrorString(e));
    for (int r = 1; r <= CEC_LOCATE_SYN_MAX && !rc; ++r) {
      if (!has_r[r]) continue;
      cec::launch_pair_syn(pp, r, 0, shard_len, vec_ok, st);
      rc = check_launch();
    }
    if (!rc) {
      cec::launch_pair_plan(pp, shard_len, 0, st);
      rc = check_launch();
    }
    for (int r = 2; r <= CEC_LOCATE_SYN_MAX && !rc; ++r) {
      if (!has_r[r]) continue;
      cec::launch_pair_syn(pp, r, 1, shard_len, vec_ok, st);
      rc = check_launch();
    }
    if (has_r[4] && !rc) {
      cec::launch_pair_plan(pp, shard_len, 1, st);
      rc = check_launch();
      if (!rc) {
        cec::launch_pair_syn(pp, 4, 2, shard_len, vec_ok, st);
        rc = check_launch();
      }
    }
    if (!rc) {
      cec::launch_pair_finish(pp, st);
      rc = check_launch();
    }
    return retire_behind(c, d, bytes, st, rc);
  }
  cec::LocatePlan lp{};
  lp.rows = dw;
  lp.sets = reinterpret_cast<const uint8_t*>(dw + sets_at);
  lp.witness = dw + wit_at;
  lp.cand = reinterpret_cast<uint32_t*>(dw + cand_at);
  lp.dirty = reinterpret_cast<uint8_t*>(dw + dirty_at);
  lp.dirty2 = lp.dirty + nseg;
  lp.flags = d_flags;
  lp.status = d_status;
  lp.rs = rs;
  lp.set_bytes = set_bytes;
  lp.nseg = (uint32_t)nseg;
  lp.n = (int)n;
  lp.k = (int)k;
  hipError_t e = hipMemsetAsync(lp.witness, 0xFF, nseg * sizeof(uint64_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(lp.dirty, 0, 2 * nseg, st);
  if (e != hipSuccess) rc = set_err(CEC_EHIP, std::string("locate preset: ") + hipGetErrorString(e));
  for (int r = 1; r <= CEC_LOCATE_SYN_MAX && !rc; ++r) {
    if (!has_r[r]) continue;
    cec::launch_syn(lp, r, false, shard_len, vec_ok, st);
    rc = check_launch();
  }
  if (!rc) {
    cec::launch_locate_plan(lp, shard_len, st);
    rc = check_launch();
  }
  for (int r = 2; r <= CEC_LOCATE_SYN_MAX && !rc; ++r) {
    if (!has_r[r]) continue;
    cec::launch_syn(lp, r, true, shard_len, vec_ok, st);
    rc = check_launch();
  }
  if (!rc) {
    cec::launch_locate_finish(lp, st);
    rc = check_launch();
  }
  if (!rc && d_nbad) {
    cec::launch_pair_nbad_single(d_status, d_nbad, nseg, st);
    rc = check_launch();
  }
  return retire_behind(c, d, bytes, st, rc);
}

int cec_locate_ptrs(cec_codec* c, const uint8_t* const* shards, size_t nseg, size_t shard_len,
                    int nsyn, uint8_t* d_flags, uint8_t* d_status, void* hip_stream) {
  if (!c || (nseg && (!shards || !d_flags || !d_status))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_locate(c->k, c->m, nsyn)) return rc;
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  return locate_impl(c, shards, nseg, shard_len, nsyn, false, d_flags, d_status, nullptr,
                     pick_stream(c, hip_stream));
}

// ---- one or two corrupt shards from parity alone (locate_multi_rule.h) -------------------------

static_assert(CEC_LOCATE_BAD_MAX == cec::kLocateBadMax, "locate_multi_rule.h states the rule");

static int check_locate_multi(int k, int m, int nsyn, int max_bad) {
  if (int rc = check_locate(k, m, nsyn)) return rc;
  if (max_bad < 1 || max_bad > CEC_LOCATE_BAD_MAX)
    return set_err(CEC_EINVAL, "max_bad must be 1..CEC_LOCATE_BAD_MAX");
  return CEC_OK;
}

int cec_locate_multi_host(int k, int m, const uint8_t* const* shards, size_t shard_len, int nsyn,
                          int max_bad, int* status, int* nfound, int found[2]) {
  if (!shards || !status || !nfound || !found) return set_err(CEC_EINVAL, "null");
  if (int rc = check_locate_multi(k, m, nsyn, max_bad)) return rc;
  uint32_t st = 0;
  if (max_bad == 1) {  // cec_locate_host's rule, its code
    int one = -1;
    cec::loc_segment_host((uint32_t)k, (uint32_t)(k + m), shards, shard_len, (uint32_t)nsyn, &st,
                          &one);
    *nfound = one >= 0 ? 1 : 0;
    found[0] = one;
    found[1] = -1;
  } else {
    cec::loc2_segment_host((uint32_t)k, (uint32_t)(k + m), shards, shard_len, (uint32_t)nsyn,
                           (uint32_t)max_bad, &st, nfound, found);
  }
  *status = (int)st;
  return CEC_OK;
}

int cec_locate_multi_ptrs(cec_codec* c, const uint8_t* const* shards, size_t nseg,
                          size_t shard_len, int nsyn, int max_bad, uint8_t* d_flags,
                          uint8_t* d_status, uint8_t* d_nbad, void* hip_stream) {
  if (!c || (nseg && (!shards || !d_flags || !d_status))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_locate_multi(c->k, c->m, nsyn, max_bad)) return rc;
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  return locate_impl(c, shards, nseg, shard_len, nsyn, max_bad >= 2, d_flags, d_status, d_nbad,
                     pick_stream(c, hip_stream));
}

int cec_reconstruct_partial_batch(cec_codec* c, uint8_t* d_data, uint8_t* d_parity, size_t nseg,
                                  size_t shard_len, const uint8_t* present, const uint8_t* held,
                                  int data_only, void* hip_stream) {
  if (!c || !present || !held || (nseg && (!d_data || !d_parity)))
    return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, hip_stream);
  const int n = c->k + c->m;
  Layout L = batch_layout(c, d_data, d_parity, shard_len);
  // per segment: n presence flags then n held flags; the same plan cache as the full rebuild
  // (the leading kind tag keeps the keys apart)
  std::string pkey(1, 'Q');
  pkey.reserve(nseg * 2 * n + 3);
  for (size_t s = 0; s < nseg; ++s) {
    for (int i = 0; i < n; ++i) pkey.push_back(present[s * n + i] ? 1 : 0);
    for (int i = 0; i < n; ++i) pkey.push_back(held[s * n + i] ? 1 : 0);
  }
  pkey.push_back(data_only ? 1 : 0);
  pkey.push_back(c->force_generic ? 1 : 0);
  return run_ps_plan(c, pkey, nseg, kPartial, data_only != 0, false, 0, L, st);
}

int cec_verify_batch(cec_codec* c, const uint8_t* d_data, const uint8_t* d_parity, size_t nseg,
                     size_t shard_len, uint8_t* d_ok, void* hip_stream) {
  if (!c || !d_ok || (nseg && (!d_data || !d_parity))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, hip_stream);
  if (!c->force_generic) {  // RS(2,1), RS(32,32): recompute and compare in one read-only pass
                            // where the layout fits (launch_verify_ct)
    Layout L = batch_layout(c, d_data, const_cast<uint8_t*>(d_parity), shard_len);
    CEC_HIP_TRY(hipMemsetAsync(d_ok, 1, nseg, st));
    if (cec::launch_verify_ct(c->k, c->m, L, d_ok, (uint32_t)nseg, st)) return check_launch();
  }
  // the parity recomputed into a scratch batch (the encode kernels: FFT for RS(32,32)), then
  // compared segment by segment with the stored parity
  const size_t pbytes = nseg * (size_t)c->m * shard_len;
  Scratch sc;
  int rc = scratch_alloc(c, pbytes, st, &sc);
  if (rc) return rc;
  void* scratch = sc.p;
  Layout L = batch_layout(c, d_data, static_cast<uint8_t*>(scratch), shard_len);
  hipError_t e = hipMemsetAsync(d_ok, 1, nseg, st);
  if (e == hipSuccess) {
    rc = do_encode(c, L, nullptr, (uint32_t)nseg, st);
    if (!rc) {
      cec::launch_cmp_segments(static_cast<const uint8_t*>(scratch), d_parity,
                               (uint64_t)c->m * shard_len, nseg, d_ok, st);
      rc = check_launch();
    }
  } else {
    rc = set_err(CEC_EHIP, std::string("verify: ") + hipGetErrorString(e));
  }
  const int mrc = c->pool.mark(st);  // the scratch stays until these launches complete
  scratch_release(c, sc, st);
  return rc ? rc : mrc;
}

int cec_xor_batch(uint8_t* d_dst, const uint8_t* d_src, size_t nsrc, size_t src_stride,
                  size_t len, void* hip_stream) {
  if ((len && nsrc && (!d_dst || !d_src)) || nsrc > 0xffffffffull)
    return set_err(CEC_EINVAL, "null buffer or too many sources");
  if (nsrc > 1 && src_stride < len)
    return set_err(CEC_EINVAL, "src_stride < len: sources overlap");
  if ((len + 255) / 256 > 0x7fffffffull) return set_err(CEC_EINVAL, "len too large (> 512 GiB)");
  if (len == 0 || nsrc == 0) return CEC_OK;
  cec::launch_xor_reduce(d_dst, d_src, (uint32_t)nsrc, src_stride, len,
                         reinterpret_cast<hipStream_t>(hip_stream));
  return check_launch();
}

// ---- what a scrub's repair proved (cec_hashq_add_check_where_ptrs's flags per segment) --------

int cec_confirm_rule(int n, int status, const uint8_t* ok, int* confirm) {
  if (n < 0 || (n && !ok) || !confirm) return set_err(CEC_EINVAL, "null or n < 0");
  uint32_t zeros = 0, ones = 0;
  for (int i = 0; i < n; ++i) {
    zeros += ok[i] == 0;
    ones += ok[i] == 1;
  }
  *confirm = (int)cec::confirm_rule(status == CEC_FLAG_REBUILT, zeros, ones);
  return CEC_OK;
}

int cec_confirm_flagged(const uint8_t* d_status, const uint8_t* d_ok, size_t nseg, int n,
                        uint8_t* d_confirm, void* hip_stream) {
  if (n < 0 || (nseg && (!d_status || !d_confirm || (n && !d_ok))))
    return set_err(CEC_EINVAL, "null buffer or n < 0");
  if (nseg / 4 > 0x7fffffffull) return set_err(CEC_EINVAL, "nseg too large");
  if (nseg == 0) return CEC_OK;
  cec::launch_confirm_flagged(d_status, d_ok, nseg, (uint32_t)n, d_confirm,
                              reinterpret_cast<hipStream_t>(hip_stream));
  return check_launch();
}

// ---- parity accumulation (EncodeIdx, Update; acc.hip) ----------------------------------------

namespace {

// Whether any of the n reads [a + s * stride, a + s * stride + len), s < n, meets [p, p + plen).
bool reads_meet(const uint8_t* a, size_t stride, size_t n, size_t len, const uint8_t* p,
                size_t plen) {
  typedef unsigned __int128 u128;
  const u128 A = (uintptr_t)a, P = (uintptr_t)p;
  u128 s = 0;  // the first read that ends past p
  if (A + len <= P) {
    if (stride == 0) return false;
    s = (P - (A + len)) / stride + 1;
  }
  return s < n && A + s * stride < P + plen;
}

// Column idx of the parity rows of E: coef[o] = E[k + o][idx].
void parity_column(const cec_codec* c, int idx, uint8_t* coef) {
  for (int o = 0; o < c->m; ++o) coef[o] = c->E->v[c->k + o][idx];
}

int check_acc_shape(size_t nseg, size_t shard_len) {
  if (int rc = check_batch(nseg, shard_len)) return rc;
  // the byte path runs ceil(shard_len / 256) blocks of 256 in x, and HIP launches fewer than 2^32
  // work items per dimension
  if ((shard_len + 255) / 256 > 0xffffffull)
    return set_err(CEC_EINVAL, "shard_len too large (> 4 GiB - 256)");
  return CEC_OK;
}

}  // namespace

int cec_encode_idx_batch(cec_codec* c, const uint8_t* d_shard, size_t shard_seg_stride, int idx,
                         uint8_t* d_parity, size_t nseg, size_t shard_len, int accumulate,
                         void* hip_stream) {
  if (!c || (nseg && (!d_shard || !d_parity))) return set_err(CEC_EINVAL, "null");
  if (idx < 0 || idx >= c->k) return set_err(CEC_EINVAL, "data shard index out of range");
  int rc = check_acc_shape(nseg, shard_len);
  if (rc) return rc;
  if (nseg > 1 && shard_seg_stride < shard_len)
    return set_err(CEC_EINVAL, "shard_seg_stride < shard_len: shards overlap");
  if (nseg == 0) return CEC_OK;
  if (reads_meet(d_shard, shard_seg_stride, nseg, shard_len, d_parity,
                 nseg * (size_t)c->m * shard_len))
    return set_err(CEC_EINVAL, "the shard overlaps the parity");
  CEC_HIP_TRY(hipSetDevice(c->device));
  uint8_t coef[cec::kMaxShards];
  parity_column(c, idx, coef);
  const uint32_t slot = 0;
  cec::launch_acc(d_shard, nullptr, shard_seg_stride, 0, d_parity, (uint64_t)c->m * shard_len,
                  shard_len, shard_len, &slot, coef, 1, c->m, accumulate != 0, nseg,
                  pick_stream(c, hip_stream));
  return check_launch();
}

int cec_update_batch(cec_codec* c, const uint8_t* d_old, const uint8_t* d_new, uint8_t* d_parity,
                     size_t nseg, size_t shard_len, const uint8_t* changed, void* hip_stream) {
  if (!c || !changed || (nseg && (!d_old || !d_new || !d_parity)))
    return set_err(CEC_EINVAL, "null");
  int rc = check_acc_shape(nseg, shard_len);
  if (rc) return rc;
  std::vector<uint32_t> slots;
  for (int j = 0; j < c->k; ++j)
    if (changed[j]) slots.push_back((uint32_t)j);
  if (nseg == 0 || slots.empty()) return CEC_OK;
  const size_t seg_stride = (size_t)c->k * shard_len, par_bytes = nseg * (size_t)c->m * shard_len;
  for (uint32_t j : slots)
    if (reads_meet(d_old + j * shard_len, seg_stride, nseg, shard_len, d_parity, par_bytes) ||
        reads_meet(d_new + j * shard_len, seg_stride, nseg, shard_len, d_parity, par_bytes))
      return set_err(CEC_EINVAL, "a changed shard overlaps the parity");
  CEC_HIP_TRY(hipSetDevice(c->device));
  std::vector<uint8_t> coef(slots.size() * c->m);
  for (size_t i = 0; i < slots.size(); ++i) parity_column(c, (int)slots[i], &coef[i * c->m]);
  cec::launch_acc(d_old, d_new, seg_stride, shard_len, d_parity, (uint64_t)c->m * shard_len,
                  shard_len, shard_len, slots.data(), coef.data(), (int)slots.size(), c->m, true,
                  nseg, pick_stream(c, hip_stream));
  return check_launch();
}

// cec_encode_idx_ptrs (in_b == NULL) and cec_update_ptrs (in_a the old bytes, in_b the new ones).
// Segments are grouped by their (input set, parity set), as reconstruct_ptrs_impl groups by
// pattern; a group's work is cut into output chunks of kRtMaxOut and input chunks of kAccMaxIn
// (chunks after the first accumulate: stream order), one launch each over the group's rows {the
// chunk's inputs [, their new bytes], the chunk's parities}. A launch's coefficients travel in its
// kernel arguments, so launches are never merged across groups.
static int acc_ptrs_impl(cec_codec* c, const uint8_t* const* in_a, const uint8_t* const* in_b,
                         uint8_t* const* parity, size_t nseg, size_t shard_len, bool accumulate,
                         void* hip_stream) {
  const int k = c->k, m = c->m;
  const bool upd = in_b != nullptr;
  if (upd)
    for (size_t i = 0; i < nseg * (size_t)k; ++i)
      if (!in_a[i] != !in_b[i])
        return set_err(CEC_EINVAL, "a data slot has one of its old and new bytes");
  struct Group {
    std::vector<int> ins, outs;
    std::vector<uint32_t> segs;
  };
  std::unordered_map<std::string, size_t> gidx;
  std::vector<Group> groups;
  std::string key((size_t)k + m, '\0');
  uintptr_t bits = 0;  // OR of every address read or written: the alignment of the call
  std::unordered_set<uintptr_t> pars;  // every parity address the call writes
  std::vector<uint8_t*> zeros;         // overwrite mode: named parity of segments that feed nothing
  for (size_t s = 0; s < nseg; ++s) {
    const uint8_t* const* dp = in_a + s * k;
    uint8_t* const* pp = parity + s * m;
    int nin = 0, nout = 0;
    for (int j = 0; j < k; ++j) nin += key[j] = dp[j] ? 1 : 0;
    for (int o = 0; o < m; ++o) nout += key[k + o] = pp[o] ? 1 : 0;
    if (!nout || (!nin && accumulate)) continue;  // no row, no work, pointers not looked at
    for (int o = 0; o < m; ++o) {
      if (!pp[o]) continue;
      if (!pars.insert((uintptr_t)pp[o]).second)
        return set_err(CEC_EINVAL, "a parity shard is named twice");
      if (nin) bits |= (uintptr_t)pp[o];
      else zeros.push_back(pp[o]);  // the encode of nothing
    }
    if (!nin) continue;
    const size_t gi = group_of(gidx, key, groups.size());
    if (gi == groups.size()) {
      Group& g = groups.emplace_back();
      for (int j = 0; j < k; ++j)
        if (key[j]) g.ins.push_back(j);
      for (int o = 0; o < m; ++o)
        if (key[k + o]) g.outs.push_back(o);
    }
    groups[gi].segs.push_back((uint32_t)s);
  }
  for (const Group& g : groups)  // inputs may repeat (they are only read), but none is a parity
    for (uint32_t s : g.segs)
      for (int j : g.ins) {
        const uintptr_t a = (uintptr_t)in_a[(size_t)s * k + j];
        const uintptr_t b = upd ? (uintptr_t)in_b[(size_t)s * k + j] : a;
        if (pars.count(a) || pars.count(b))
          return set_err(CEC_EINVAL, "a parity shard is an input of the call");
        bits |= a | b;
      }
  if (groups.empty() && zeros.empty()) return CEC_OK;
  const bool vec_ok = (bits & 15) == 0;
  struct Coefs {
    int nin, nout;
    bool accumulate;
    std::vector<uint8_t> coef;  // [nin][nout]
  };
  std::vector<Coefs> coefs;
  std::vector<PtrLaunch> launches;
  for (const Group& g : groups) {
    const int nin = (int)g.ins.size(), nout = (int)g.outs.size();
    for (int o0 = 0; o0 < nout; o0 += cec::kRtMaxOut) {
      const int no = std::min(nout - o0, cec::kRtMaxOut);
      for (int j0 = 0; j0 < nin; j0 += cec::kAccMaxIn) {
        const int ni = std::min(nin - j0, cec::kAccMaxIn);
        Coefs cf{ni, no, accumulate || j0 > 0, std::vector<uint8_t>((size_t)ni * no)};
        for (int j = 0; j < ni; ++j)
          for (int o = 0; o < no; ++o)
            cf.coef[(size_t)j * no + o] = c->E->v[k + g.outs[o0 + o]][g.ins[j0 + j]];
        PtrLaunch l{PtrKind::acc, cec::rt_bucket(no), (uint32_t)((upd ? 2 : 1) * ni + no), {},
                    (int)coefs.size()};
        l.rows.reserve(g.segs.size() * l.rs);
        for (uint32_t s : g.segs) {
          for (int j = 0; j < ni; ++j)
            l.rows.push_back((uint64_t)(uintptr_t)in_a[(size_t)s * k + g.ins[j0 + j]]);
          if (upd)
            for (int j = 0; j < ni; ++j)
              l.rows.push_back((uint64_t)(uintptr_t)in_b[(size_t)s * k + g.ins[j0 + j]]);
          for (int o = 0; o < no; ++o)
            l.rows.push_back((uint64_t)(uintptr_t)parity[(size_t)s * m + g.outs[o0 + o]]);
        }
        coefs.push_back(std::move(cf));
        launches.push_back(std::move(l));
      }
    }
  }
  CEC_HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, hip_stream);
  Uploads up{c->stream, c->arena};
  int rc = run_ptr_table(c, launches, up, st, [] { return (int)CEC_OK; },
                         [&](const PtrLaunch& l, const uint64_t* tab, uint32_t nrows) {
                           const Coefs& cf = coefs[l.id];
                           cec::launch_acc_ptrs(tab, nrows, cf.coef.data(), cf.nin, cf.nout, upd,
                                                cf.accumulate, shard_len, vec_ok, st);
                         });
  return clear_shards(rc, zeros, shard_len, st, "encode_idx");
}

int cec_encode_idx_ptrs(cec_codec* c, const uint8_t* const* data, uint8_t* const* parity,
                        size_t nseg, size_t shard_len, int accumulate, void* hip_stream) {
  if (!c || (nseg && (!data || !parity))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_acc_shape(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  return acc_ptrs_impl(c, data, nullptr, parity, nseg, shard_len, accumulate != 0, hip_stream);
}

int cec_update_ptrs(cec_codec* c, const uint8_t* const* old_data, const uint8_t* const* new_data,
                    uint8_t* const* parity, size_t nseg, size_t shard_len, void* hip_stream) {
  if (!c || (nseg && (!old_data || !new_data || !parity))) return set_err(CEC_EINVAL, "null");
  if (int rc = check_acc_shape(nseg, shard_len)) return rc;
  if (nseg == 0) return CEC_OK;
  return acc_ptrs_impl(c, old_data, new_data, parity, nseg, shard_len, true, hip_stream);
}

int cec_sha256_batch(cec_codec* c, const uint8_t* d_data, const uint8_t* d_parity, size_t nseg,
                     size_t shard_len, uint8_t* d_hex, void* hip_stream) {
  if (!c || !d_hex || (nseg && !d_data)) return set_err(CEC_EINVAL, "null");
  CEC_HIP_TRY(hipSetDevice(c->device));
  Layout L = batch_layout(c, d_data, d_parity, shard_len);
  int nsh = c->k + c->m;
  if (!d_parity) {
    nsh = c->k;
    L.parity = nullptr;
  }
  cec::launch_sha256_hex(c->opts.sha_mode, nullptr, &L, nsh, (uint64_t)nseg * nsh, shard_len,
                         d_hex, pick_stream(c, hip_stream));
  return check_launch();
}

int cec_sha256_hex(const uint8_t* const* d_bufs, size_t n, size_t len, uint8_t* hex,
                   void* hip_stream) {
  if (!hex || (n && !d_bufs)) return set_err(CEC_EINVAL, "null");
  if (n == 0) return CEC_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const uint8_t** dptrs = nullptr;
  uint8_t* dhex = nullptr;
  // stream-ordered (hipFree would synchronise the whole device)
  CEC_HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&dptrs), n * sizeof(void*), st));
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&dhex), n * 64, st);
  if (e != hipSuccess) {
    (void)hipFreeAsync(dptrs, st);
    return set_err(CEC_ENOMEM, "hex buffer");
  }
  int rc = CEC_OK;
  do {
    if ((e = hipMemcpyAsync(dptrs, d_bufs, n * sizeof(void*), hipMemcpyHostToDevice, st))) break;
    cec::launch_sha256_hex(0, dptrs, nullptr, 1, n, len, dhex, st);
    if ((e = hipGetLastError())) break;
    if ((e = hipMemcpyAsync(hex, dhex, n * 64, hipMemcpyDeviceToHost, st))) break;
    e = hipStreamSynchronize(st);
  } while (0);
  if (e != hipSuccess) rc = set_err(CEC_EHIP, std::string("sha256: ") + hipGetErrorString(e));
  (void)hipFreeAsync(dptrs, st);
  (void)hipFreeAsync(dhex, st);
  return rc;
}

int cec_split_segment(const uint8_t* seg, size_t seg_len, int k, uint8_t* const* shards,
                      size_t shard_len) {
  if (!shards || k < 1) return set_err(CEC_EINVAL, "null shards or k < 1");
  if (seg_len == 0 || !seg) return set_err(CEC_ESHORTDATA, "empty segment");
  if (shard_len == 0 || (size_t)k * shard_len < seg_len)
    return set_err(CEC_ESHARDLEN, "k * shard_len < seg_len");
  for (int i = 0; i < k; ++i) {
    if (!shards[i]) return set_err(CEC_EINVAL, "null shard");
    const size_t off = (size_t)i * shard_len;
    const size_t take = off >= seg_len ? 0 : std::min(shard_len, seg_len - off);
    if (take) std::memcpy(shards[i], seg + off, take);
    if (take < shard_len) std::memset(shards[i] + take, 0, shard_len - take);
  }
  return CEC_OK;
}

int cec_fill_synthetic(uint8_t* d_out, size_t seg_bytes, size_t nseg, uint64_t seg0,
                       uint64_t seed, void* hip_stream) {
  if (!d_out && nseg) return set_err(CEC_EINVAL, "null");
  if (seg_bytes % 8) return set_err(CEC_EINVAL, "seg_bytes must be a multiple of 8");
  if (nseg == 0 || seg_bytes == 0) return CEC_OK;
  cec::launch_fill_splitmix(d_out, seg_bytes, nseg, seg0, seed,
                            reinterpret_cast<hipStream_t>(hip_stream));
  return check_launch();
}

// ---- storage audit chunks -----------------------------------------------------------------

int cec_challenge_indices(const uint64_t* randoms, size_t nrand, uint32_t chunk_count,
                          uint32_t need, uint32_t* out, size_t* used) {
  if ((nrand && !randoms) || (need && !out)) return set_err(CEC_EINVAL, "null");
  if (chunk_count == 0 || need > chunk_count)
    return set_err(CEC_EINVAL, "need must be <= chunk_count, chunk_count > 0");
  // c-pallets/audit/src/lib.rs:955-964
  uint32_t got = 0;
  size_t i = 0;
  for (; i < nrand && got < need; ++i) {
    const uint32_t idx = (uint32_t)(randoms[i] % chunk_count);
    bool seen = false;
    for (uint32_t q = 0; q < got && !seen; ++q) seen = out[q] == idx;
    if (!seen) out[got++] = idx;
  }
  if (used) *used = i;
  if (got < need) return set_err(CEC_EINVAL, "random stream exhausted before `need` indices");
  return CEC_OK;
}

int cec_audit_chunks(cec_codec* c, const uint8_t* d_data, const uint8_t* d_parity, size_t nseg,
                     size_t shard_len, uint32_t chunk_count, const uint32_t* indices,
                     uint32_t nidx, uint8_t* d_chunks, uint8_t* d_hex, void* hip_stream) {
  if (!c || !indices || (nseg && !d_data) || (!d_chunks && !d_hex))
    return set_err(CEC_EINVAL, "null");
  if (chunk_count == 0 || shard_len == 0 || shard_len % chunk_count)
    return set_err(CEC_ESHARDLEN, "shard_len must be a nonzero multiple of chunk_count");
  for (uint32_t j = 0; j < nidx; ++j)
    if (indices[j] >= chunk_count) return set_err(CEC_EINVAL, "chunk index out of range");
  if (nseg == 0 || nidx == 0) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, hip_stream);
  const int nsh = d_parity ? c->k + c->m : c->k;
  const uint64_t nfrag = (uint64_t)nseg * nsh;
  const uint64_t chunk = shard_len / chunk_count;
  Layout L = batch_layout(c, d_data, d_parity, shard_len);
  void* d_idx = nullptr;
  int rc = c->pool.alloc(nidx * sizeof(uint32_t), &d_idx);
  if (rc) return rc;
  const size_t idx_bytes = nidx * sizeof(uint32_t);
  hipError_t e = hipMemcpyAsync(d_idx, indices, idx_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    c->pool.retire(d_idx, idx_bytes);
    return set_err(CEC_EHIP, std::string("index upload: ") + hipGetErrorString(e));
  }
  Scratch sc;
  const size_t gbytes = nfrag * nidx * chunk;
  if (!d_chunks) {
    rc = scratch_alloc(c, gbytes, st, &sc);
    if (rc) {
      c->pool.retire(d_idx, idx_bytes);
      return rc;
    }
    d_chunks = static_cast<uint8_t*>(sc.p);
  }
  cec::launch_chunk_gather(L, nsh, nfrag, static_cast<const uint32_t*>(d_idx), nidx, chunk,
                           d_chunks, st);
  rc = check_launch();
  if (!rc && d_hex) {
    Layout G{};  // the gathered chunks as nfrag * nidx one-shard "segments"
    G.data = d_chunks;
    G.len = chunk;
    G.shard_stride = chunk;
    G.data_seg_stride = chunk;
    G.k = 1;
    cec::launch_sha256_hex(c->opts.sha_mode, nullptr, &G, 1, nfrag * nidx, chunk, d_hex, st);
    rc = check_launch();
  }
  const int mrc = c->pool.mark(st);  // the index array and scratch stay until these complete
  c->pool.retire(d_idx, idx_bytes);
  scratch_release(c, sc, st);
  return rc ? rc : mrc;
}

int cec_audit_chunks_ptrs(cec_codec* c, const uint8_t* const* frags, size_t nfrag,
                          size_t shard_len, uint32_t chunk_count, const uint32_t* indices,
                          uint32_t nidx, uint8_t* d_chunks, uint8_t* d_hex, void* hip_stream) {
  if (!c || (!d_chunks && !d_hex)) return set_err(CEC_EINVAL, "null");
  if (chunk_count == 0 || shard_len == 0 || shard_len % chunk_count)
    return set_err(CEC_ESHARDLEN, "shard_len must be a nonzero multiple of chunk_count");
  if (nfrag == 0 || nidx == 0) return CEC_OK;
  if (!frags || !indices) return set_err(CEC_EINVAL, "null");
  for (uint32_t j = 0; j < nidx; ++j)
    if (indices[j] >= chunk_count) return set_err(CEC_EINVAL, "chunk index out of range");
  const uint64_t chunk = shard_len / chunk_count;
  uintptr_t bits = (uintptr_t)d_chunks | chunk;
  for (size_t f = 0; f < nfrag; ++f) {
    if (!frags[f]) return set_err(CEC_EINVAL, "null fragment");
    if (frags[f] == d_chunks || frags[f] == d_hex)
      return set_err(CEC_EINVAL, "an output is a fragment of the call");
    bits |= (uintptr_t)frags[f];
  }
  // one chain index and one table word per chunk, both 32-bit counted in the kernels; grid x
  if (nfrag > 0xFFFFFFFFull / nidx) return set_err(CEC_EINVAL, "too many chunks (>= 2^32)");
  const bool vec_ok = (bits & 15) == 0;
  const uint64_t per_tile = vec_ok ? 256 * 16 : 256;
  if ((chunk + per_tile - 1) / per_tile * nidx > 0x7fffffffull)
    return set_err(CEC_EINVAL, "nidx * chunk too large for one grid");
  CEC_HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, hip_stream);
  // Address tables only, in one pool block: the fragment addresses (8 bytes each), the indices
  // (4 bytes each, padded to a word) and, for the hashes, one address per chunk, filled on the
  // device. No chunk byte is copied for the hashes and nothing chunk-sized is allocated.
  const size_t nchunks = nfrag * nidx;
  const size_t idx_words = ((size_t)nidx + 1) / 2;
  const size_t up_words = nfrag + idx_words;
  const size_t bytes = (up_words + (d_hex ? nchunks : 0)) * sizeof(uint64_t);
  std::vector<uint64_t> host(up_words, 0);
  for (size_t f = 0; f < nfrag; ++f) host[f] = (uint64_t)(uintptr_t)frags[f];
  std::memcpy(host.data() + nfrag, indices, nidx * sizeof(uint32_t));
  void* d = nullptr;
  int rc = c->pool.alloc(bytes, &d);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(d, host.data(), up_words * sizeof(uint64_t),
                                hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    c->pool.retire(d, bytes);
    return set_err(CEC_EHIP, std::string("table upload: ") + hipGetErrorString(e));
  }
  const uint64_t* d_frags = static_cast<const uint64_t*>(d);
  const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(d_frags + nfrag);
  uint64_t* d_addrs = static_cast<uint64_t*>(d) + up_words;
  if (d_chunks) {
    cec::launch_chunk_gather_tab(d_frags, nfrag, d_idx, nidx, chunk, d_chunks, vec_ok, st);
    rc = check_launch();
  }
  if (!rc && d_hex) {
    // hashed where they lie, also when the chunks are gathered: the same bytes either way
    cec::launch_chunk_addrs(d_frags, nfrag, d_idx, nidx, chunk, d_addrs, st);
    rc = check_launch();
    if (!rc) {
      cec::launch_sha256_hex(c->opts.sha_mode, reinterpret_cast<const uint8_t* const*>(d_addrs),
                             nullptr, 1, nchunks, chunk, d_hex, st);
      rc = check_launch();
    }
  }
  const int mrc = c->pool.mark(st);  // the tables stay until these complete
  c->pool.retire(d, bytes);
  return rc ? rc : mrc;
}

// ---- host-buffer API -------------------------------------------------------------------

int cec_encode(cec_codec* c, uint8_t* const* shards, size_t shard_len) {
  if (!c || !shards) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(1, shard_len)) return rc;
  const int n = c->k + c->m;
  for (int i = 0; i < n; ++i)
    if (!shards[i]) return set_err(CEC_EINVAL, "null shard");
  CEC_HIP_TRY(hipSetDevice(c->device));
  int rc = stage_ensure(c, n, shard_len);
  if (rc) return rc;
  Layout L = stage_layout(c, shard_len);
  if ((rc = stage_up(c, L.data, shards, c->k, shard_len))) return rc;
  rc = do_encode(c, L, nullptr, 1, c->stream);
  if (rc) return rc;
  if ((rc = stage_down(c, shards + c->k, L.parity, c->m, shard_len))) return rc;
  CEC_HIP_TRY(hipStreamSynchronize(c->stream));
  return CEC_OK;
}

int cec_reconstruct(cec_codec* c, uint8_t* const* shards, const uint8_t* present,
                    size_t shard_len, int data_only) {
  if (!c || !shards || !present) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(1, shard_len)) return rc;
  const int n = c->k + c->m;
  CEC_HIP_TRY(hipSetDevice(c->device));
  ProgPtr p;
  int rc = get_decode(c, present, data_only != 0, &p);
  if (rc) return rc;
  if (p->nout == 0) return CEC_OK;
  for (int i = 0; i < n; ++i)
    if (!shards[i]) return set_err(CEC_EINVAL, "null shard");
  const size_t stride = pad256(shard_len);
  rc = stage_ensure(c, n, shard_len);
  if (rc) return rc;
  Layout L = stage_layout(c, shard_len);
  // Upload only the survivors the plan reads.
  for (int j = 0; j < c->k; ++j) {
    const int i = p->in_idx[j];
    if ((rc = stage_up(c, c->stage + i * stride, shards + i, 1, shard_len))) return rc;
  }
  rc = do_decode(c, *p, L, nullptr, 1, c->stream);
  if (rc) return rc;
  for (int o = 0; o < p->nout; ++o) {
    const int i = p->out_idx[o];
    if ((rc = stage_down(c, shards + i, c->stage + i * stride, 1, shard_len))) return rc;
  }
  CEC_HIP_TRY(hipStreamSynchronize(c->stream));
  evict_decode(c);  // the launch above has completed
  return CEC_OK;
}

int cec_verify(cec_codec* c, uint8_t* const* shards, size_t shard_len, int* ok) {
  if (!c || !shards || !ok) return set_err(CEC_EINVAL, "null");
  if (int rc = check_batch(1, shard_len)) return rc;
  const int n = c->k + c->m;
  for (int i = 0; i < n; ++i)
    if (!shards[i]) return set_err(CEC_EINVAL, "null shard");
  CEC_HIP_TRY(hipSetDevice(c->device));
  int rc = stage_ensure(c, n, shard_len);
  if (rc) return rc;
  Layout L = stage_layout(c, shard_len);
  if ((rc = stage_up(c, L.data, shards, c->k, shard_len))) return rc;
  rc = do_encode(c, L, nullptr, 1, c->stream);
  if (rc) return rc;
  std::vector<uint8_t> par(shard_len);
  uint8_t* const host = par.data();
  *ok = 1;
  for (int o = 0; o < c->m && *ok; ++o) {
    if ((rc = stage_down(c, &host, L.parity + o * L.shard_stride, 1, shard_len))) return rc;
    CEC_HIP_TRY(hipStreamSynchronize(c->stream));
    if (std::memcmp(par.data(), shards[c->k + o], shard_len) != 0) *ok = 0;
  }
  return CEC_OK;
}

// Stages only what is read: [the shard][m parity shards], shards at stride pad256(len).
int cec_encode_idx(cec_codec* c, const uint8_t* data_shard, int idx, uint8_t* const* parity,
                   size_t shard_len) {
  if (!c || !data_shard || !parity) return set_err(CEC_EINVAL, "null");
  if (idx < 0 || idx >= c->k) return set_err(CEC_EINVAL, "data shard index out of range");
  int rc = check_acc_shape(1, shard_len);
  if (rc) return rc;
  for (int o = 0; o < c->m; ++o)
    if (!parity[o]) return set_err(CEC_EINVAL, "null parity shard");
  CEC_HIP_TRY(hipSetDevice(c->device));
  const size_t stride = pad256(shard_len);
  rc = stage_ensure(c, 1 + (size_t)c->m, shard_len);
  if (rc) return rc;
  uint8_t* d_par = c->stage + stride;
  if ((rc = stage_up(c, c->stage, &data_shard, 1, shard_len))) return rc;
  if ((rc = stage_up(c, d_par, parity, c->m, shard_len))) return rc;
  uint8_t coef[cec::kMaxShards];
  parity_column(c, idx, coef);
  const uint32_t slot = 0;
  cec::launch_acc(c->stage, nullptr, 0, 0, d_par, 0, stride, shard_len, &slot, coef, 1, c->m, true,
                  1, c->stream);
  rc = check_launch();
  if (rc) return rc;
  if ((rc = stage_down(c, parity, d_par, c->m, shard_len))) return rc;
  CEC_HIP_TRY(hipStreamSynchronize(c->stream));
  return CEC_OK;
}

// Stages [old bytes of the changed shards][their new bytes][m parity shards].
int cec_update(cec_codec* c, uint8_t* const* shards, const uint8_t* const* new_data,
               size_t shard_len) {
  if (!c || !shards || !new_data) return set_err(CEC_EINVAL, "null");
  int rc = check_acc_shape(1, shard_len);
  if (rc) return rc;
  std::vector<int> ch;
  for (int j = 0; j < c->k; ++j) {
    if (!new_data[j]) continue;
    if (!shards[j]) return set_err(CEC_EINVAL, "new data for a shard whose old bytes are missing");
    ch.push_back(j);
  }
  for (int o = 0; o < c->m; ++o)
    if (!shards[c->k + o]) return set_err(CEC_EINVAL, "null parity shard");
  if (ch.empty()) return CEC_OK;
  CEC_HIP_TRY(hipSetDevice(c->device));
  const size_t stride = pad256(shard_len), nc = ch.size();
  rc = stage_ensure(c, 2 * nc + (size_t)c->m, shard_len);
  if (rc) return rc;
  uint8_t* d_new = c->stage + nc * stride;
  uint8_t* d_par = c->stage + 2 * nc * stride;
  std::vector<uint32_t> slots(nc);
  std::vector<uint8_t> coef(nc * c->m);
  for (size_t i = 0; i < nc; ++i) {
    if ((rc = stage_up(c, c->stage + i * stride, shards + ch[i], 1, shard_len))) return rc;
    if ((rc = stage_up(c, d_new + i * stride, new_data + ch[i], 1, shard_len))) return rc;
    slots[i] = (uint32_t)i;
    parity_column(c, ch[i], &coef[i * c->m]);
  }
  if ((rc = stage_up(c, d_par, shards + c->k, c->m, shard_len))) return rc;
  cec::launch_acc(c->stage, d_new, 0, stride, d_par, 0, stride, shard_len, slots.data(),
                  coef.data(), (int)nc, c->m, true, 1, c->stream);
  rc = check_launch();
  if (rc) return rc;
  if ((rc = stage_down(c, shards + c->k, d_par, c->m, shard_len))) return rc;
  CEC_HIP_TRY(hipStreamSynchronize(c->stream));
  return CEC_OK;
}

}  // extern "C"
