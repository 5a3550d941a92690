// group.cpp - the device group: RCCL loader, the followers' host threads, pack / ship / gather of the members' tiles, ovr_hip_create_group.
#include "state.hpp"

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>

using namespace ovrhip;
using namespace ovrhip::host;

// ---- the followers' host threads --------------------------------------------------------------------------------------------------
// One per follower, created with the group, pinned to the member's device once (hipSetDevice is per thread).  The leader's thread posts a
// command to every worker and waits for all of them: the members' commits, frame launches, packs and frame ends run side by side.  A worker
// spins on its mailbox for a short while after a command (a render loop posts the next one within microseconds) and then sleeps on a
// condition variable; results travel back in the mailbox (g_last_error is thread-local).  (Global like ovr_hip_renderer, whose state names it.)
struct GroupWorker {
  ovr_hip_renderer* m = nullptr;
  std::thread th;
  std::mutex mx;
  std::condition_variable cv;
  std::atomic<uint64_t> posted{ 0 }, done{ 0 };
  std::atomic<bool> asleep{ false };
  int cmd = GW_NONE;          // written by the leader before `posted` advances, read by the worker after it has seen it
  std::function<int()> fn;    // GW_CALL
  int rc = 0;                 // the command's result ...
  std::string err;            // ... and its message
};

namespace ovrhip {
namespace host {

// ------------------------------------------------------------------------------------------------------------------
// Device group: the image-plane shard of SURVEY.md 8e INSIDE one process, behind the same handle - what the reference's unmodified
// apps reach through the plugin (north_star: "apps run unmodified ... the 8 GPUs of one node shard the image plane into
// tiles with a final RCCL gather over xGMI").  Every member renders its own tiles of the frame on its own device (volume replicated,
// TEA seeds by global pixel index: the assembled frame is the single-GPU frame bit for bit); at the end of the frame each follower packs
// its tiles, its comm_stream ships them to the leader's device - ncclSend / ncclRecv over RCCL's communicators of this process
// (ncclCommInitAll) when the devices are distinct, peer-to-peer copies otherwise (OVR_HIP_GATHER=rccl|copy forces one) - and the leader
// scatters all payloads into its framebuffer with one launch per layer.  mapframe / swap / accumulation work on the leader's
// framebuffer as with one device.  The reference has one device (device_impl.cpp:371-372) and nothing to mirror here.
// ------------------------------------------------------------------------------------------------------------------
struct RcclApi { // resolved at run time: libovr_hip.so does not link RCCL, a host without it falls back to peer copies
  void* lib = nullptr;
  int (*CommInitAll)(void**, int, const int*) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
static const RcclApi& rccl_api()
{
  static const RcclApi api = [] {
    RcclApi a;
    for (const char* name : { "librccl.so.1", "librccl.so" })
      if ((a.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    if (!a.lib) return a;
    a.CommInitAll = (int (*)(void**, int, const int*))dlsym(a.lib, "ncclCommInitAll");
    a.CommDestroy = (int (*)(void*))dlsym(a.lib, "ncclCommDestroy");
    a.GroupStart = (int (*)())dlsym(a.lib, "ncclGroupStart");
    a.GroupEnd = (int (*)())dlsym(a.lib, "ncclGroupEnd");
    a.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(a.lib, "ncclSend");
    a.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(a.lib, "ncclRecv");
    a.GetErrorString = (const char* (*)(int))dlsym(a.lib, "ncclGetErrorString");
    a.ok = a.CommInitAll && a.CommDestroy && a.GroupStart && a.GroupEnd && a.Send && a.Recv;
    return a;
  }();
  return api;
}
constexpr int kNcclFloat = 7; // ncclFloat32, rccl.h

// (re)size the payload and gather buffers for the committed framebuffer size and tiles
static int group_buffers(ovr_hip_renderer* L)
{
  const int n = (int)L->group.members.size();
  const ShardP& s0 = L->shard.current;
  const int W = L->fbsize.current.w, H = L->fbsize.current.h;
  if (L->group.fb[0] == W && L->group.fb[1] == H && L->group.fb[2] == s0.tw && L->group.fb[3] == s0.th && L->group.fb[4] == n) return 0;
  size_t most = 0;
  for (int i = 0; i < n; ++i) {
    ovr_hip_renderer* m = L->group.members[i];
    const size_t px = (size_t)count_owned_tiles(W, H, s0.tw, s0.th, i, n) * s0.tw * s0.th;
    most = std::max(most, px);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->group.comm_stream));
    for (int c = 0; c < 2; ++c) {
      if (m->group.d_payload[c]) HIP_TRY(hipFree(m->group.d_payload[c]));
      m->group.d_payload[c] = nullptr;
      m->group.payload_floats[c] = px * (c == 0 ? 4 : 3);
      if (i > 0 && px > 0 && (c == 0 || L->group.grad)) HIP_TRY(hipMalloc((void**)&m->group.d_payload[c], m->group.payload_floats[c] * sizeof(float)));
    }
  }
  HIP_TRY(hipSetDevice(L->device));
  for (int c = 0; c < 2; ++c) {
    if (L->group.d_gather[c]) HIP_TRY(hipFree(L->group.d_gather[c]));
    L->group.d_gather[c] = nullptr;
    L->group.stride[c] = ((most * (c == 0 ? 4 : 3) + 11) / 12) * 12; // floats; a multiple of 3 and of 4: whole pixels in either layer
    if (most > 0 && (c == 0 || L->group.grad)) HIP_TRY(hipMalloc((void**)&L->group.d_gather[c], L->group.stride[c] * (size_t)n * sizeof(float)));
  }
  L->group.fb[0] = W; L->group.fb[1] = H; L->group.fb[2] = s0.tw; L->group.fb[3] = s0.th; L->group.fb[4] = n;
  return 0;
}

static int group_pack(ovr_hip_renderer* L, ovr_hip_renderer* m);

static inline void cpu_relax() { __builtin_ia32_pause(); }

static void group_worker_main(GroupWorker* w)
{
  ovr_hip_renderer* m = w->m;
  (void)hipSetDevice(m->device);
  uint64_t seen = 0;
  static const int spin_us = getenv("OVR_HIP_WORKER_SPIN_US") ? atoi(getenv("OVR_HIP_WORKER_SPIN_US")) : 200;
  for (;;) {
    // wait for the next command: spin first (the render loop's next post is microseconds away), then sleep
    const auto t0 = std::chrono::steady_clock::now();
    int polls = 0;
    while (w->posted.load(std::memory_order_acquire) == seen) {
      cpu_relax();
      if ((++polls & 255) == 0 && std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > spin_us) {
        std::unique_lock<std::mutex> lk(w->mx);
        w->asleep.store(true);
        w->cv.wait(lk, [&] { return w->posted.load() != seen; });
        w->asleep.store(false);
      }
    }
    seen = w->posted.load(std::memory_order_acquire);
    int rc = 0;
    g_last_error.clear();
    switch (w->cmd) {
    case GW_COMMIT: rc = ovr_hip_commit(m); break;
    case GW_RENDER: rc = ovr_hip_render_async(m); break;
    case GW_SHIP: rc = group_pack(m->group.leader, m); break;
    case GW_FINISH: rc = finish_frame_one(m); break;
    case GW_SWAP: rc = ovr_hip_swap(m); break;
    case GW_CALL: rc = w->fn ? w->fn() : 0; break;
    case GW_QUIT: w->done.store(seen, std::memory_order_release); return;
    default: break;
    }
    w->rc = rc;
    if (rc) w->err = g_last_error;
    w->done.store(seen, std::memory_order_release);
  }
}

static void gw_post(GroupWorker* w, int cmd)
{
  w->cmd = cmd;
  w->posted.fetch_add(1); // (seq_cst: ordered against the worker's `asleep` store - either it sees the post or this thread sees it asleep)
  if (w->asleep.load()) {
    std::lock_guard<std::mutex> lk(w->mx);
    w->cv.notify_one();
  }
}
static int gw_wait(GroupWorker* w)
{
  const uint64_t want = w->posted.load();
  int polls = 0;
  while (w->done.load(std::memory_order_acquire) != want) {
    cpu_relax();
    if ((++polls & 4095) == 0) std::this_thread::yield();
  }
  if (w->rc) g_last_error = w->err;
  return w->rc;
}
// the same command on every follower, the leader's own share (if any) meanwhile on this thread; the first error wins, every worker is waited for
int group_run(ovr_hip_renderer* L, int cmd, const std::function<int()>& own)
{
  const size_t n = L->group.members.size();
  for (size_t i = 1; i < n; ++i) gw_post(L->group.members[i]->group.worker, cmd);
  int e = own ? own() : 0;
  std::string msg = e ? g_last_error : std::string();
  for (size_t i = 1; i < n; ++i) {
    const int ei = gw_wait(L->group.members[i]->group.worker);
    if (ei && !e) { e = ei; msg = g_last_error; }
  }
  if (e) g_last_error = msg;
  return e;
}
// an arbitrary call per follower (volume upload, noise tile: rare, may allocate), `own` meanwhile on this thread
int group_call(ovr_hip_renderer* L, const std::function<int(ovr_hip_renderer*)>& f, const std::function<int()>& own)
{
  const size_t n = L->group.members.size();
  for (size_t i = 1; i < n; ++i) {
    ovr_hip_renderer* m = L->group.members[i];
    m->group.worker->fn = [m, &f] { return f(m); };
  }
  return group_run(L, GW_CALL, own);
}
void group_stop_workers(ovr_hip_renderer* L)
{
  for (size_t i = 1; i < L->group.members.size(); ++i) {
    GroupWorker* w = L->group.members[i]->group.worker;
    if (!w) continue;
    if (w->th.joinable()) { gw_post(w, GW_QUIT); w->th.join(); }
    delete w;
    L->group.members[i]->group.worker = nullptr;
  }
}

// follower m (on its own thread): pack the tiles of the frame in flight (or just finished) behind it; with peer copies the payload leaves at once
// on m's comm_stream (ends in m->group.ev_shipped), with RCCL it waits in m->group.d_payload for the leader's grouped send / recv (group_rccl)
static int group_pack(ovr_hip_renderer* L, ovr_hip_renderer* m)
{
  const int W = L->fbsize.current.w, H = L->fbsize.current.h;
  const ShardP& s = m->shard.current;
  m->group.shipped_by_rccl = false;
  if (m->group.payload_floats[0] == 0) { HIP_TRY(hipEventRecord(m->group.ev_shipped, m->group.comm_stream)); return 0; }
  // ovr_hip_pack_tiles resolves a frame whose request pool is not yet known to be roomy before it packs (a pool overflow renders the frame again)
  if (int e = ovr_hip_pack_tiles(m, m->group.d_payload[0], m->group.payload_floats[0] * sizeof(float))) return e;
  if (L->group.grad) HIP_TRY(launch_pack_tiles(m->d_grad[m->cur], m->group.d_payload[1], W, H, s.tw, s.th, s.rank, s.world, m->stream(), 3));
  HIP_TRY(hipEventRecord(m->group.ev_packed, m->stream()));
  HIP_TRY(hipStreamWaitEvent(m->group.comm_stream, m->group.ev_packed, 0));
  if (L->group.gather_kind == 2) return 0;
  for (int c = 0; c < 2; ++c) {
    if (c == 1 && !L->group.grad) break;
    float* dst = L->group.d_gather[c] + (size_t)m->group.rank * L->group.stride[c];
    if (m->device == L->device) HIP_TRY(hipMemcpyAsync(dst, m->group.d_payload[c], m->group.payload_floats[c] * sizeof(float), hipMemcpyDeviceToDevice, m->group.comm_stream));
    else HIP_TRY(hipMemcpyPeerAsync(dst, L->device, m->group.d_payload[c], m->device, m->group.payload_floats[c] * sizeof(float), m->group.comm_stream));
  }
  HIP_TRY(hipEventRecord(m->group.ev_shipped, m->group.comm_stream));
  return 0;
}

// leader thread, RCCL: the payloads of the listed followers travel inside ONE ncclGroupStart / End - n - 1 sends on the followers' communicators and
// comm streams, n - 1 receives on the leader's - and the leader's comm_stream records ONE event behind them (round 4 issued a group per follower: 7
// launch pairs a frame at 8 members, each receive queued behind the slowest member packed before it).  false = RCCL refused: the caller falls back.
static bool group_rccl(ovr_hip_renderer* L, const std::vector<ovr_hip_renderer*>& who)
{
  const RcclApi& N = rccl_api();
  if (hipSetDevice(L->device) != hipSuccess) return false;
  // the receives start once every listed payload exists (a receive kernel spinning beside the leader's own frame would only take CUs from it)
  for (ovr_hip_renderer* m : who)
    if (m->group.payload_floats[0] > 0 && hipStreamWaitEvent(L->group.comm_stream, m->group.ev_packed, 0) != hipSuccess) return false;
  int rc = N.GroupStart();
  for (size_t k = 0; k < who.size() && rc == 0; ++k) {
    ovr_hip_renderer* m = who[k];
    if (m->group.payload_floats[0] == 0) continue;
    for (int c = 0; c < 2 && rc == 0; ++c) {
      if (c == 1 && !L->group.grad) break;
      (void)hipSetDevice(m->device);
      rc = N.Send(m->group.d_payload[c], m->group.payload_floats[c], kNcclFloat, 0, m->group.rccl_comm, m->group.comm_stream);
      (void)hipSetDevice(L->device);
      if (rc == 0) rc = N.Recv(L->group.d_gather[c] + (size_t)m->group.rank * L->group.stride[c], m->group.payload_floats[c], kNcclFloat, m->group.rank, L->group.rccl_comm, L->group.comm_stream);
    }
  }
  const int rc2 = N.GroupEnd();
  (void)hipSetDevice(L->device);
  if (rc != 0 || rc2 != 0) {
    fprintf(stderr, "[hip] RCCL send / recv of a device group's tiles failed (%s): the group goes on with peer copies\n", N.GetErrorString ? N.GetErrorString(rc != 0 ? rc : rc2) : "?");
    return false;
  }
  if (hipEventRecord(L->group.ev_gathered, L->group.comm_stream) != hipSuccess) return false;
  for (ovr_hip_renderer* m : who) m->group.shipped_by_rccl = true;
  return true;
}

// packs (workers, side by side) and ships the tiles of the listed followers; `all` = every follower (the common case: one post per worker)
static int group_ship(ovr_hip_renderer* L, const std::vector<ovr_hip_renderer*>& who, bool all)
{
  auto pack = [&]() -> int {
    if (all) return group_run(L, GW_SHIP);
    for (ovr_hip_renderer* m : who) gw_post(m->group.worker, GW_SHIP);
    int e = 0;
    std::string msg;
    for (ovr_hip_renderer* m : who) { const int ei = gw_wait(m->group.worker); if (ei && !e) { e = ei; msg = g_last_error; } }
    if (e) g_last_error = msg;
    return e;
  };
  if (int e = pack()) return e;
  if (L->group.gather_kind == 2 && !group_rccl(L, who)) {
    L->group.gather_kind = 1; // same bytes, same destination, by peer copies from here on
    (void)hipGetLastError();
    if (int e = pack()) return e;
  }
  return 0;
}

static int group_finish(ovr_hip_renderer* L)
{
  const int n = (int)L->group.members.size();
  bool any = L->async_pending;
  for (int i = 1; i < n; ++i) any = any || L->group.members[i]->async_pending;
  if (!any) return 0;
  const int W = L->fbsize.current.w, H = L->fbsize.current.h;
  if (int e = group_buffers(L)) return e;
  const auto t0 = std::chrono::high_resolution_clock::now();
  // 1. the followers pack behind their frames and ship on their comm streams while everything still renders
  std::vector<ovr_hip_renderer*> followers(L->group.members.begin() + 1, L->group.members.end());
  if (int e = group_ship(L, followers, true)) return e;
  const auto t1 = std::chrono::high_resolution_clock::now();
  // 2. every frame to its end (a follower whose request pool overflowed renders again: its early payload is stale)
  if (int e = group_run(L, GW_FINISH, [&] { return finish_frame_one(L); })) return e;
  std::vector<ovr_hip_renderer*> stale;
  for (ovr_hip_renderer* m : followers)
    if (m->stats.stale_tiles) stale.push_back(m);
  if (!stale.empty())
    if (int e = group_ship(L, stale, false)) return e;
  const auto t2 = std::chrono::high_resolution_clock::now();
  // 3. the leader scatters the payloads into the framebuffer set the frame rendered into
  hipStream_t st = L->stream();
  bool waited_rccl = false;
  for (ovr_hip_renderer* m : followers) {
    if (!m->group.shipped_by_rccl) HIP_TRY(hipStreamWaitEvent(st, m->group.ev_shipped, 0));
    else if (!waited_rccl) { HIP_TRY(hipStreamWaitEvent(st, L->group.ev_gathered, 0)); waited_rccl = true; } // (recorded behind the LAST grouped receive: covers a re-shipment too)
  }
  const ShardP& s = L->shard.current;
  if (W > 0 && H > 0 && L->group.d_gather[0]) {
    HIP_TRY(launch_unpack_tiles(L->group.d_gather[0], L->d_rgba[L->frame_set], W, H, s.tw, s.th, -1, n, L->group.stride[0], st, 4, 0));
    if (L->group.grad && L->group.d_gather[1]) HIP_TRY(launch_unpack_tiles(L->group.d_gather[1], L->d_grad[L->frame_set], W, H, s.tw, s.th, -1, n, L->group.stride[1], st, 3, 0));
  }
  HIP_TRY(hipStreamSynchronize(st));
  const auto t3 = std::chrono::high_resolution_clock::now();
  L->group.gather_ms = std::chrono::duration<double, std::milli>(t3 - t2).count();
  L->group.host_us[1] = std::chrono::duration<double, std::micro>(t1 - t0).count();
  L->group.host_us[2] = std::chrono::duration<double, std::micro>(t2 - t1).count();
  L->group.host_us[3] = std::chrono::duration<double, std::micro>(t3 - t2).count();
  // 4. the frame's counters: sums over the members, times of the slowest
  L->group.own_stats = L->stats;
  for (int i = 1; i < n; ++i) {
    const ovr_hip_stats& a = L->group.members[i]->stats;
    ovr_hip_stats& t = L->stats;
    t.rays += a.rays; t.samples += a.samples; t.shaded_samples += a.shaded_samples; t.shadow_samples += a.shadow_samples;
    t.active_pixels += a.active_pixels; t.skipped_samples += a.skipped_samples; t.skipped_shadow_samples += a.skipped_shadow_samples;
    t.pool_chunks += a.pool_chunks;
    t.kernel_ms = std::max(t.kernel_ms, a.kernel_ms); t.march_ms = std::max(t.march_ms, a.march_ms);
    t.shade_ms = std::max(t.shade_ms, a.shade_ms); t.composite_ms = std::max(t.composite_ms, a.composite_ms);
    t.replicas_building += a.replicas_building;
    if (a.tuning == 1) t.tuning = 1;
    if (L->group.members[i]->outside_hits) { // a hit through an ignored slab on any member: the leader's set is mapped whole (see finish_frame_one)
      L->map_whole_set(L->frame_set);
    }
  }
  L->stats.stale_tiles = 0;
  return 0;
}

int finish_frame(ovr_hip_renderer* r)
{
  if (r->group.members.size() > 1) return group_finish(r);
  return finish_frame_one(r);
}
// what a renderer holds as a member of a group (ovr_hip_destroy, on the renderer's device)
void group_release(ovr_hip_renderer* r)
{
  if (r->group.rccl_comm && rccl_api().ok) (void)rccl_api().CommDestroy(r->group.rccl_comm);
  for (int c = 0; c < 2; ++c) {
    if (r->group.d_payload[c]) (void)hipFree(r->group.d_payload[c]);
    if (r->group.d_gather[c]) (void)hipFree(r->group.d_gather[c]);
  }
  if (r->group.comm_stream) (void)hipStreamDestroy(r->group.comm_stream);
  if (r->group.ev_packed) (void)hipEventDestroy(r->group.ev_packed);
  if (r->group.ev_shipped) (void)hipEventDestroy(r->group.ev_shipped);
  if (r->group.ev_received) (void)hipEventDestroy(r->group.ev_received);
  if (r->group.ev_gathered) (void)hipEventDestroy(r->group.ev_gathered);
}

} // namespace host
} // namespace ovrhip

extern "C" {

int ovr_hip_create_group(ovr_hip_renderer** out, const int32_t* device_ids, int32_t n_devices)
{
  if (!out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_create_group: null output pointer");
  *out = nullptr;
  if (!device_ids || n_devices < 1 || n_devices > 64) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_create_group: 1 to 64 device ordinals expected");
  ovr_hip_renderer* L = nullptr;
  if (int e = ovr_hip_create(&L, device_ids[0])) return e;
  if (n_devices == 1) { *out = L; return 0; } // one device: an ordinary renderer
  L->group.members.push_back(L);
  auto build = [&]() -> int {
    for (int i = 1; i < n_devices; ++i) {
      ovr_hip_renderer* m = nullptr;
      if (int e = ovr_hip_create(&m, device_ids[i])) return e;
      m->group.leader = L;
      m->group.rank = i;
      L->group.members.push_back(m);
    }
    int tw = 16, th = 16; // measured work max / mean over 8 ranks 1.07 (1.33 with 64 x 64): DESIGN.md section 5
    if (const char* t = getenv("OVR_HIP_TILE")) { int a = 0, b = 0; if (sscanf(t, "%dx%d", &a, &b) == 2 && a > 0 && b > 0) { tw = a; th = b; } }
    bool distinct = true;
    for (int i = 0; i < n_devices; ++i)
      for (int j = 0; j < i; ++j) distinct = distinct && device_ids[i] != device_ids[j];
    for (int i = 0; i < n_devices; ++i) {
      ovr_hip_renderer* m = L->group.members[i];
      HIP_TRY(hipSetDevice(m->device));
      HIP_TRY(hipStreamCreateWithFlags(&m->group.comm_stream, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&m->group.ev_packed, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&m->group.ev_shipped, hipEventDisableTiming));
      if (i > 0) {
        HIP_TRY(hipSetDevice(L->device));
        HIP_TRY(hipEventCreateWithFlags(&m->group.ev_received, hipEventDisableTiming));
        HIP_TRY(hipSetDevice(m->device));
      }
      ShardP s; s.rank = i; s.world = n_devices; s.tw = tw; s.th = th;
      m->shard.current = m->shard.queued = s;
      m->sched.list_dirty = true;
      for (int j = 0; j < n_devices; ++j) // direct xGMI / PCIe peer access where the platform has it (the copies work without, staged by the runtime)
        if (device_ids[j] != m->device) { int can = 0; if (hipDeviceCanAccessPeer(&can, m->device, device_ids[j]) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(device_ids[j], 0); }
      (void)hipGetLastError(); // hipErrorPeerAccessAlreadyEnabled is not an error
    }
    HIP_TRY(hipSetDevice(L->device));
    HIP_TRY(hipEventCreateWithFlags(&L->group.ev_gathered, hipEventDisableTiming));
    if (const char* g = getenv("OVR_HIP_MAP_GRAD")) L->group.grad = g[0] != '0';
    const char* want = getenv("OVR_HIP_GATHER");
    const bool force_rccl = want && std::string(want) == "rccl", force_copy = want && std::string(want) == "copy";
    if (want && !force_rccl && !force_copy) return fail(OVR_HIP_EINVAL, "[hip] OVR_HIP_GATHER must be 'rccl' or 'copy'");
    L->group.gather_kind = 1;
    if (!force_copy && distinct && rccl_api().ok) { // one communicator per device of this process (ncclCommInitAll refuses a device listed twice)
      std::vector<void*> comms((size_t)n_devices, nullptr);
      std::vector<int> devs(device_ids, device_ids + n_devices);
      const int rc = rccl_api().CommInitAll(comms.data(), n_devices, devs.data());
      if (rc == 0) {
        for (int i = 0; i < n_devices; ++i) L->group.members[i]->group.rccl_comm = comms[(size_t)i];
        L->group.gather_kind = 2;
      }
      else if (force_rccl) return fail(OVR_HIP_EDEVICE, std::string("[hip] ncclCommInitAll failed: ") + (rccl_api().GetErrorString ? rccl_api().GetErrorString(rc) : "?"));
      HIP_TRY(hipSetDevice(L->device));
    }
    else if (force_rccl) return fail(OVR_HIP_EDEVICE, distinct ? "[hip] OVR_HIP_GATHER=rccl but librccl.so could not be loaded" : "[hip] OVR_HIP_GATHER=rccl needs distinct devices (RCCL refuses a device listed twice)");
    // one host thread per follower (round 5): device set once, persistent - commits, frame launches, packs and frame ends of the members run side by side
    for (int i = 1; i < n_devices; ++i) {
      GroupWorker* w = new GroupWorker();
      w->m = L->group.members[i];
      L->group.members[i]->group.worker = w;
      try { w->th = std::thread(group_worker_main, w); }
      catch (const std::exception& ex) { return fail(OVR_HIP_EDEVICE, std::string("[hip] ovr_hip_create_group: no host thread for a member: ") + ex.what()); }
    }
    // the first multi-GPU run explains itself: which way the tiles travel and why, and what the platform says about every pair
    if (!(getenv("OVR_HIP_QUIET") && atoi(getenv("OVR_HIP_QUIET")) != 0)) {
      std::string why = L->group.gather_kind == 2 ? "RCCL send / recv (ncclCommInitAll over the listed devices; one ncclGroupStart / End per frame)"
                        : force_copy       ? "peer copies (OVR_HIP_GATHER=copy)"
                        : !distinct        ? "peer copies (a device is listed more than once: RCCL refuses that)"
                        : !rccl_api().ok   ? "peer copies (librccl.so could not be loaded)"
                                           : "peer copies (ncclCommInitAll failed)";
      std::string devs, peers;
      for (int i = 0; i < n_devices; ++i) { char d[16]; snprintf(d, sizeof(d), "%s%d", i ? "," : "", device_ids[i]); devs += d; }
      for (int i = 0; i < n_devices; ++i) {
        peers += i ? " | " : "";
        for (int j = 0; j < n_devices; ++j) {
          int can = device_ids[i] == device_ids[j] ? 1 : 0;
          if (!can && hipDeviceCanAccessPeer(&can, device_ids[i], device_ids[j]) != hipSuccess) { (void)hipGetLastError(); can = -1; }
          peers += can < 0 ? "?" : can ? "1" : "0";
        }
      }
      fprintf(stderr, "[hip] device group: devices [%s], image tiles %dx%d, gather to device %d by %s; gradient layer %s; hipDeviceCanAccessPeer rows (member -> member): %s\n",
              devs.c_str(), tw, th, device_ids[0], why.c_str(), L->group.grad ? "travels too" : "stays (OVR_HIP_MAP_GRAD=0)", peers.c_str());
    }
    return 0;
  };
  if (int e = build()) { const std::string msg = g_last_error; ovr_hip_destroy(L); g_last_error = msg; return e; }
  *out = L;
  return 0;
}

// The RCCL entry points a device group uses, exercised on ONE device: a communicator of one rank (ncclCommInitAll), a send to itself matched by
// a receive inside one ncclGroupStart / End on a stream, the payload compared.  A device group's own RCCL branch needs distinct devices; this
// pins what can be pinned on one card - the library resolves, the prototypes and the data-type constant are right, the calls run on a stream.
int ovr_hip_rccl_selftest(int device_id)
{
  const RcclApi& N = rccl_api();
  if (!N.ok) return fail(OVR_HIP_ESTATE, "[hip] librccl.so could not be loaded (a device group then gathers with peer copies)");
  HIP_TRY(hipSetDevice(device_id));
  void* comm = nullptr;
  const int dev = device_id;
  int rc = N.CommInitAll(&comm, 1, &dev);
  if (rc != 0) return fail(OVR_HIP_EDEVICE, std::string("[hip] ncclCommInitAll(1 device) failed: ") + (N.GetErrorString ? N.GetErrorString(rc) : "?"));
  const size_t n = 1 << 16;
  float *src = nullptr, *dst = nullptr;
  hipStream_t st = nullptr;
  std::vector<float> h(n), back(n, -1.f);
  for (size_t i = 0; i < n; ++i) h[i] = (float)i * 0.25f;
  auto run = [&]() -> int {
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_TRY(hipMalloc((void**)&src, n * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&dst, n * sizeof(float)));
    HIP_TRY(hipMemcpy(src, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dst, 0, n * sizeof(float)));
    int a = N.GroupStart();
    if (a == 0) a = N.Send(src, n, kNcclFloat, 0, comm, st);
    if (a == 0) a = N.Recv(dst, n, kNcclFloat, 0, comm, st);
    const int b = N.GroupEnd();
    if (a != 0 || b != 0) return fail(OVR_HIP_EDEVICE, std::string("[hip] RCCL self send / recv failed: ") + (N.GetErrorString ? N.GetErrorString(a != 0 ? a : b) : "?"));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(back.data(), dst, n * sizeof(float), hipMemcpyDeviceToHost));
    if (std::memcmp(back.data(), h.data(), n * sizeof(float)) != 0) return fail(OVR_HIP_EDEVICE, "[hip] RCCL self send / recv delivered other bytes than were sent");
    return 0;
  };
  const int e = run();
  const std::string msg = g_last_error;
  if (src) (void)hipFree(src);
  if (dst) (void)hipFree(dst);
  if (st) (void)hipStreamDestroy(st);
  (void)N.CommDestroy(comm);
  g_last_error = msg;
  return e;
}

int ovr_hip_group_info(const ovr_hip_renderer* r, int32_t* n_devices, int32_t* gather_kind, double* gather_ms)
{
  if (!r) return fail(OVR_HIP_EINVAL, "[hip] null renderer");
  if (n_devices) *n_devices = r->group.members.size() > 1 ? (int32_t)r->group.members.size() : 1;
  if (gather_kind) *gather_kind = r->group.members.size() > 1 ? r->group.gather_kind : 0;
  if (gather_ms) *gather_ms = r->group.members.size() > 1 ? r->group.gather_ms : 0.0;
  return 0;
}

int ovr_hip_group_host_times(const ovr_hip_renderer* r, double out_us[4])
{
  if (!r || !out_us) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_group_host_times: null argument");
  for (int i = 0; i < 4; ++i) out_us[i] = r->group.members.size() > 1 ? r->group.host_us[i] : 0.0;
  return 0;
}

int ovr_hip_get_member_stats(const ovr_hip_renderer* r, int32_t member, ovr_hip_stats* out)
{
  if (!r || !out) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_member_stats: null argument");
  const int n = r->group.members.size() > 1 ? (int)r->group.members.size() : 1;
  if (member < 0 || member >= n) return fail(OVR_HIP_EINVAL, "[hip] ovr_hip_get_member_stats: no such member");
  if (r->async_pending) return fail(OVR_HIP_ESTATE, "[hip] ovr_hip_get_member_stats: a frame is still in flight (call ovr_hip_sync)");
  *out = n > 1 ? (member == 0 ? r->group.own_stats : r->group.members[(size_t)member]->stats) : r->stats;
  return 0;
}

} // extern "C"
