// mpi4jax_amd native bridge: RCCL collectives enqueued on the current HIP
// stream, operating zero-copy on torch tensor buffers in HBM3E.
//
// This replaces the reference's CUDA FFI backend
// (/root/reference/mpi4jax/_src/xla_bridge/mpi_xla_bridge_cuda.cpp), whose
// GPU path was stream-synchronize + host MPI (optionally staging every
// buffer through host malloc, :185-206).  Here there is NO stream
// synchronize and NO staging: ncclAllReduce & friends are enqueued directly
// on the stream torch compute runs on, so ordering against compute is free
// and the wire rate is xGMI, not PCIe-to-host.
//
// Communicator registry: int64 keys -> {ncclComm_t, scratch}, mirroring the
// reference's int64 handle marshalling idea (mpi_ops_common.h:36-48) but
// into our own registry instead of raw MPI handles.

#include <torch/extension.h>
#include <torch/version.h>

#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>

#include "halo_geom.h"
#include "kernels.h"

namespace {

#define HIP_CHECK(cmd)                                                       \
  do {                                                                       \
    hipError_t e_ = (cmd);                                                   \
    TORCH_CHECK(e_ == hipSuccess, "HIP error: ", hipGetErrorString(e_),      \
                " at " __FILE__ ":", __LINE__);                              \
  } while (0)

// Abort-on-error discipline mirrors the reference (mpi_ops_common.h:60-78):
// a failed collective leaves the communicator unusable, so surface the
// error loudly.  We throw into Python instead of MPI_Abort so tests can
// assert on it; an unhandled throw still kills the rank.
#define RCCL_CHECK(cmd)                                                      \
  do {                                                                       \
    ncclResult_t r_ = (cmd);                                                 \
    TORCH_CHECK(r_ == ncclSuccess, "RCCL error: ", ncclGetErrorString(r_),   \
                " in " #cmd);                                                \
  } while (0)

struct CommEntry {
  ncclComm_t comm = nullptr;
  int rank = -1;
  int size = 0;
  void* barrier_buf = nullptr;  // persistent 4-byte scratch for barrier
};

std::mutex g_mutex;
std::unordered_map<int64_t, CommEntry> g_comms;
int64_t g_next_id = 1;
bool g_logging = false;

CommEntry get_comm(int64_t id) {  // by value: entries are tiny PODs and a
  // reference would dangle if another thread destroyed the comm
  std::lock_guard<std::mutex> lk(g_mutex);
  auto it = g_comms.find(id);
  TORCH_CHECK(it != g_comms.end(), "unknown RCCL communicator handle ", id);
  return it->second;
}

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

ncclDataType_t nccl_dtype(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kChar: return ncclInt8;
    case at::kByte: return ncclUint8;
    case at::kBool: return ncclUint8;
    case at::kInt: return ncclInt32;
    case at::kLong: return ncclInt64;
    case at::kHalf: return ncclFloat16;
    case at::kFloat: return ncclFloat32;
    case at::kDouble: return ncclFloat64;
    case at::kBFloat16: return ncclBfloat16;
    default:
      TORCH_CHECK(false, "dtype ", t.scalar_type(),
                  " not supported by the RCCL backend");
  }
}

int dt_code(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return DT_F32;
    case at::kDouble: return DT_F64;
    case at::kHalf: return DT_F16;
    case at::kBFloat16: return DT_BF16;
    case at::kChar: return DT_I8;
    case at::kByte: return DT_U8;
    case at::kBool: return DT_U8;
    case at::kInt: return DT_I32;
    case at::kLong: return DT_I64;
    default:
      TORCH_CHECK(false, "dtype ", t.scalar_type(),
                  " not supported by device combine kernels");
  }
}

void check_pair(const at::Tensor& out, const at::Tensor& in) {
  TORCH_CHECK(in.is_cuda() && out.is_cuda(),
              "RCCL backend requires device tensors");
  TORCH_CHECK(in.is_contiguous() && out.is_contiguous(),
              "RCCL backend requires contiguous tensors");
  TORCH_CHECK(in.scalar_type() == out.scalar_type(), "dtype mismatch");
}

void log_enqueue(const char* op, const CommEntry& c, int64_t items) {
  if (g_logging) {
    std::printf("r%d | native   | %s enqueue (%lld items)\n", c.rank, op,
                (long long)items);
    std::fflush(stdout);
  }
}

// -------------------------------------------------------------- watchdog
// Opt-in fail-fast for wedged communication (reference abort discipline:
// mpi_ops_common.h:60-78).  RCCL enqueues asynchronously, so a mismatched
// send/recv never fails — it silently wedges the stream forever.  With
// MPI4JAX_AMD_WATCHDOG_SEC > 0 every collective enqueue records a stream
// event; a monitor thread aborts all communicators and exits the process
// (rank-tagged stderr, exit code 87) if an event is still pending past
// the deadline.  Off by default: event record costs ~2 us per enqueue.
struct WatchEntry {
  hipEvent_t ev;
  std::chrono::steady_clock::time_point deadline;
  const char* what;  // static strings only
  int rank;
};

std::atomic<double> g_watchdog_sec{0.0};
std::atomic<bool> g_watch_run{false};
// leaked on purpose: a detached monitor thread may outlive static dtors
std::mutex* g_watch_mu = new std::mutex;
std::deque<WatchEntry>* g_watch = new std::deque<WatchEntry>;

void watch_loop() {
  using clock = std::chrono::steady_clock;
  while (g_watch_run.load(std::memory_order_relaxed)) {
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    std::lock_guard<std::mutex> lk(*g_watch_mu);
    for (auto it = g_watch->begin(); it != g_watch->end();) {
      hipError_t q = hipEventQuery(it->ev);
      if (q == hipSuccess) {
        (void)hipEventDestroy(it->ev);
        it = g_watch->erase(it);
        continue;
      }
      if (clock::now() > it->deadline) {
        std::fprintf(stderr,
                     "[mpi4jax_amd r%d] WATCHDOG: %s still pending after "
                     "%.1fs — aborting all RCCL communicators and exiting "
                     "(mismatched send/recv or a dead peer wedged the "
                     "stream)\n",
                     it->rank, it->what, g_watchdog_sec.load());
        std::fflush(stderr);
        {
          std::lock_guard<std::mutex> ck(g_mutex);
          for (auto& kv : g_comms) ncclCommAbort(kv.second.comm);
        }
        std::_Exit(87);
      }
      ++it;
    }
  }
}

void watchdog_arm(const char* what, int rank, hipStream_t stream) {
  double t = g_watchdog_sec.load(std::memory_order_relaxed);
  if (t <= 0) return;
  hipEvent_t ev;
  HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(ev, stream));
  auto deadline = std::chrono::steady_clock::now() +
                  std::chrono::duration_cast<
                      std::chrono::steady_clock::duration>(
                      std::chrono::duration<double>(t));
  std::lock_guard<std::mutex> lk(*g_watch_mu);
  g_watch->push_back({ev, deadline, what, rank});
}

void set_watchdog(double seconds) {
  g_watchdog_sec.store(seconds);
  if (seconds > 0 && !g_watch_run.exchange(true)) {
    std::thread(watch_loop).detach();
  }
}

double get_watchdog() { return g_watchdog_sec.load(); }

// test-only: wedge the current stream with a BOUNDED spin kernel so the
// watchdog's abort path can be exercised at world 1 (RCCL self-mismatches
// error synchronously there; real wedges need a peer).  Self-terminates
// after `seconds` so a failed watchdog cannot hold the GPU past the test
// timeout.  wall_clock64 ticks at the fixed ~100 MHz wall clock.
__global__ void debug_spin_kernel(long long ticks) {
  long long start = wall_clock64();
  while (wall_clock64() - start < ticks) __builtin_amdgcn_s_sleep(63);
}

void debug_wedge_stream(double seconds) {
  if (seconds > 120.0) seconds = 120.0;
  long long ticks = (long long)(seconds * 1.0e8);
  hipLaunchKernelGGL(debug_spin_kernel, dim3(1), dim3(1), 0, cur_stream(),
                     ticks);
  watchdog_arm("debug_wedge", -1, cur_stream());
}

// roctx range around every collective enqueue — shows up in
// `rocprofv3 --marker-trace` timelines (tracing spans)
struct RoctxRange {
  explicit RoctxRange(const char* name) { roctxRangePushA(name); }
  ~RoctxRange() { roctxRangePop(); }
};
#define ROCTX_SCOPE(name) RoctxRange roctx_scope_(name)

// ---------------------------------------------------------------- lifecycle

py::bytes get_unique_id() {
  ncclUniqueId id;
  RCCL_CHECK(ncclGetUniqueId(&id));
  return py::bytes(reinterpret_cast<const char*>(&id), sizeof(id));
}

int64_t comm_init_rank(int64_t nranks, int64_t rank, py::bytes uid_bytes) {
  std::string uid_str = uid_bytes;
  TORCH_CHECK(uid_str.size() == sizeof(ncclUniqueId),
              "bad ncclUniqueId size ", uid_str.size());
  ncclUniqueId uid;
  std::memcpy(&uid, uid_str.data(), sizeof(uid));
  ncclComm_t comm;
  {
    // init is collective across ranks; release the GIL so ranks can meet
    py::gil_scoped_release nogil;
    RCCL_CHECK(ncclCommInitRank(&comm, (int)nranks, uid, (int)rank));
  }
  CommEntry e;
  e.comm = comm;
  e.rank = (int)rank;
  e.size = (int)nranks;
  HIP_CHECK(hipMalloc(&e.barrier_buf, 8));
  HIP_CHECK(hipMemset(e.barrier_buf, 0, 8));
  std::lock_guard<std::mutex> lk(g_mutex);
  int64_t id = g_next_id++;
  g_comms[id] = e;
  return id;
}

void comm_destroy(int64_t id) {
  std::lock_guard<std::mutex> lk(g_mutex);
  auto it = g_comms.find(id);
  if (it == g_comms.end()) return;
  ncclCommDestroy(it->second.comm);
  (void)hipFree(it->second.barrier_buf);
  g_comms.erase(it);
}

void destroy_all_comms() {
  std::lock_guard<std::mutex> lk(g_mutex);
  for (auto& kv : g_comms) {
    ncclCommDestroy(kv.second.comm);
    (void)hipFree(kv.second.barrier_buf);
  }
  g_comms.clear();
}

int64_t comm_count() {
  std::lock_guard<std::mutex> lk(g_mutex);
  return (int64_t)g_comms.size();
}

// async-error surfacing: RCCL collectives are enqueued asynchronously, so
// a transport failure shows up later on the communicator.  The reference's
// failure model is fail-fast abort (mpi_ops_common.h:60-78); here
// check_async_errors() is called from flush()/finalize() and can be called
// by users — it throws if any communicator has failed.
void check_async_errors() {
  std::lock_guard<std::mutex> lk(g_mutex);
  for (auto& kv : g_comms) {
    ncclResult_t st = ncclSuccess;
    ncclCommGetAsyncError(kv.second.comm, &st);
    TORCH_CHECK(st == ncclSuccess, "RCCL communicator ", kv.first,
                " failed asynchronously: ", ncclGetErrorString(st));
  }
}

void comm_abort(int64_t id) {
  std::lock_guard<std::mutex> lk(g_mutex);
  auto it = g_comms.find(id);
  if (it == g_comms.end()) return;
  ncclCommAbort(it->second.comm);
  (void)hipFree(it->second.barrier_buf);
  g_comms.erase(it);
}

// user-buffer registration (RCCL >= 2.19): lets RCCL use zero-copy
// protocols on registered persistent buffers (multi-GPU bandwidth win)
int64_t comm_register(int64_t comm_id, at::Tensor buf) {
  auto c = get_comm(comm_id);
  TORCH_CHECK(buf.is_cuda() && buf.is_contiguous(), "bad buffer");
  void* handle = nullptr;
  RCCL_CHECK(ncclCommRegister(c.comm, buf.data_ptr(),
                              buf.numel() * buf.element_size(), &handle));
  return (int64_t)(uintptr_t)handle;
}

void comm_deregister(int64_t comm_id, int64_t handle) {
  auto c = get_comm(comm_id);
  RCCL_CHECK(ncclCommDeregister(c.comm, (void*)(uintptr_t)handle));
}

void set_logging(bool enabled) { g_logging = enabled; }

py::dict version_info() {
  py::dict d;
  int nccl_ver = 0;
  ncclGetVersion(&nccl_ver);
  d["rccl"] = nccl_ver;
  int hip_ver = 0;
  (void)hipRuntimeGetVersion(&hip_ver);
  d["hip_runtime"] = hip_ver;
  return d;
}

// what this .so was COMPILED against — the runtime side (version_info)
// is compared against this at import (the reference's runtime-vs-build
// MPI ABI check, xla_bridge/__init__.py:23-89, re-expressed for the
// torch-C++-ABI + RCCL pair that matters here)
py::dict build_info() {
  py::dict d;
  d["torch"] = std::to_string(TORCH_VERSION_MAJOR) + "." +
               std::to_string(TORCH_VERSION_MINOR) + "." +
               std::to_string(TORCH_VERSION_PATCH);
  d["rccl_header"] =
      NCCL_MAJOR * 10000 + NCCL_MINOR * 100 + NCCL_PATCH;
  d["glibcxx_use_cxx11_abi"] = (int)_GLIBCXX_USE_CXX11_ABI;
  return d;
}

// --------------------------------------------------------------- collectives

void allreduce(at::Tensor out, at::Tensor in, int64_t op, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::allreduce");
  auto c = get_comm(comm_id);
  check_pair(out, in);
  TORCH_CHECK(out.numel() == in.numel(), "size mismatch");
  log_enqueue("Allreduce", c, in.numel());
  RCCL_CHECK(ncclAllReduce(in.data_ptr(), out.data_ptr(), in.numel(),
                           nccl_dtype(in), (ncclRedOp_t)op, c.comm,
                           cur_stream()));
  watchdog_arm("allreduce", c.rank, cur_stream());
}

void reduce(at::Tensor out, at::Tensor in, int64_t op, int64_t root,
            int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::reduce");
  auto c = get_comm(comm_id);
  check_pair(out, in);
  log_enqueue("Reduce", c, in.numel());
  RCCL_CHECK(ncclReduce(in.data_ptr(), out.data_ptr(), in.numel(),
                        nccl_dtype(in), (ncclRedOp_t)op, (int)root, c.comm,
                        cur_stream()));
  watchdog_arm("reduce", c.rank, cur_stream());
}

void allgather(at::Tensor out, at::Tensor in, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::allgather");
  auto c = get_comm(comm_id);
  check_pair(out, in);
  TORCH_CHECK(out.numel() == in.numel() * c.size, "allgather size mismatch");
  log_enqueue("Allgather", c, in.numel());
  RCCL_CHECK(ncclAllGather(in.data_ptr(), out.data_ptr(), in.numel(),
                           nccl_dtype(in), c.comm, cur_stream()));
  watchdog_arm("allgather", c.rank, cur_stream());
}

void broadcast(at::Tensor out, at::Tensor in, int64_t root, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::bcast");
  auto c = get_comm(comm_id);
  check_pair(out, in);
  log_enqueue("Bcast", c, in.numel());
  RCCL_CHECK(ncclBroadcast(in.data_ptr(), out.data_ptr(), in.numel(),
                           nccl_dtype(in), (int)root, c.comm, cur_stream()));
  watchdog_arm("bcast", c.rank, cur_stream());
}

void reduce_scatter(at::Tensor out, at::Tensor in, int64_t op,
                    int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::reduce_scatter");
  auto c = get_comm(comm_id);
  check_pair(out, in);
  TORCH_CHECK(in.numel() == out.numel() * c.size,
              "reduce_scatter size mismatch");
  log_enqueue("ReduceScatter", c, in.numel());
  RCCL_CHECK(ncclReduceScatter(in.data_ptr(), out.data_ptr(), out.numel(),
                               nccl_dtype(in), (ncclRedOp_t)op, c.comm,
                               cur_stream()));
  watchdog_arm("reduce_scatter", c.rank, cur_stream());
}


// RCCL's collectives take size_t counts, but point-to-point transfers
// silently truncate somewhere above 2^31 elements (observed on RCCL
// 2.26: the tail of an 8.6 GB ncclSend/Recv pair never arrives).  All
// p2p goes through these chunked wrappers; chunking is deterministic so
// both sides of a pair split identically inside the group.
constexpr int64_t kP2PChunk = int64_t(1) << 30;  // elements

void p2p_send(const void* ptr, int64_t count, ncclDataType_t dt,
              size_t esz, int peer, ncclComm_t comm, hipStream_t stream) {
  const char* p = (const char*)ptr;
  while (count > 0) {
    int64_t c = count < kP2PChunk ? count : kP2PChunk;
    RCCL_CHECK(ncclSend(p, c, dt, peer, comm, stream));
    p += c * esz;
    count -= c;
  }
}

void p2p_recv(void* ptr, int64_t count, ncclDataType_t dt, size_t esz,
              int peer, ncclComm_t comm, hipStream_t stream) {
  char* p = (char*)ptr;
  while (count > 0) {
    int64_t c = count < kP2PChunk ? count : kP2PChunk;
    RCCL_CHECK(ncclRecv(p, c, dt, peer, comm, stream));
    p += c * esz;
    count -= c;
  }
}

// grouped p2p composition: RCCL has no alltoall/gather/scatter primitives
//  — on the fully-connected xGMI clique direct per-peer
// send/recv IS the bandwidth-optimal algorithm (every peer pair has its own
// 153 GB/s link; no forwarding needed).

void alltoall(at::Tensor out, at::Tensor in, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::alltoall");
  auto c = get_comm(comm_id);
  check_pair(out, in);
  TORCH_CHECK(in.numel() % c.size == 0, "alltoall count not divisible");
  int64_t chunk = in.numel() / c.size;
  int64_t esz = in.element_size();
  auto dt = nccl_dtype(in);
  char* ip = (char*)in.data_ptr();
  char* op_ = (char*)out.data_ptr();
  log_enqueue("Alltoall", c, in.numel());
  RCCL_CHECK(ncclGroupStart());
  for (int r = 0; r < c.size; ++r) {
    p2p_send(ip + r * chunk * esz, chunk, dt, esz, r, c.comm,
             cur_stream());
    p2p_recv(op_ + r * chunk * esz, chunk, dt, esz, r, c.comm,
             cur_stream());
  }
  RCCL_CHECK(ncclGroupEnd());
  watchdog_arm("alltoall", c.rank, cur_stream());
}

void gather(at::Tensor out, at::Tensor in, int64_t root, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::gather");
  auto c = get_comm(comm_id);
  TORCH_CHECK(in.is_cuda() && in.is_contiguous(), "bad gather input");
  int64_t chunk = in.numel();
  int64_t esz = in.element_size();
  auto dt = nccl_dtype(in);
  log_enqueue("Gather", c, chunk);
  RCCL_CHECK(ncclGroupStart());
  p2p_send(in.data_ptr(), chunk, dt, esz, (int)root, c.comm,
           cur_stream());
  if (c.rank == (int)root) {
    TORCH_CHECK(out.numel() == chunk * c.size, "gather out size mismatch");
    char* op_ = (char*)out.data_ptr();
    for (int r = 0; r < c.size; ++r) {
      p2p_recv(op_ + r * chunk * esz, chunk, dt, esz, r, c.comm,
               cur_stream());
    }
  }
  RCCL_CHECK(ncclGroupEnd());
  watchdog_arm("gather", c.rank, cur_stream());
}

void scatter(at::Tensor out, at::Tensor in, int64_t root, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::scatter");
  auto c = get_comm(comm_id);
  TORCH_CHECK(out.is_cuda() && out.is_contiguous(), "bad scatter output");
  int64_t chunk = out.numel();
  int64_t esz = out.element_size();
  auto dt = nccl_dtype(out);
  log_enqueue("Scatter", c, chunk);
  RCCL_CHECK(ncclGroupStart());
  if (c.rank == (int)root) {
    TORCH_CHECK(in.numel() == chunk * c.size, "scatter in size mismatch");
    char* ip = (char*)in.data_ptr();
    for (int r = 0; r < c.size; ++r) {
      p2p_send(ip + r * chunk * esz, chunk, dt, esz, r, c.comm,
               cur_stream());
    }
  }
  p2p_recv(out.data_ptr(), chunk, dt, esz, (int)root, c.comm,
           cur_stream());
  RCCL_CHECK(ncclGroupEnd());
  watchdog_arm("scatter", c.rank, cur_stream());
}

void send(at::Tensor in, int64_t dest, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::send");
  auto c = get_comm(comm_id);
  TORCH_CHECK(in.is_cuda() && in.is_contiguous(), "bad send input");
  log_enqueue("Send", c, in.numel());
  p2p_send(in.data_ptr(), in.numel(), nccl_dtype(in), in.element_size(),
           (int)dest, c.comm, cur_stream());
  watchdog_arm("send", c.rank, cur_stream());
}

void recv(at::Tensor out, int64_t source, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::recv");
  auto c = get_comm(comm_id);
  TORCH_CHECK(out.is_cuda() && out.is_contiguous(), "bad recv output");
  log_enqueue("Recv", c, out.numel());
  p2p_recv(out.data_ptr(), out.numel(), nccl_dtype(out),
           out.element_size(), (int)source, c.comm, cur_stream());
  watchdog_arm("recv", c.rank, cur_stream());
}

void sendrecv(at::Tensor sendbuf, at::Tensor recvbuf, int64_t source,
              int64_t dest, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::sendrecv");
  auto c = get_comm(comm_id);
  TORCH_CHECK(sendbuf.is_cuda() && sendbuf.is_contiguous(), "bad sendbuf");
  TORCH_CHECK(recvbuf.is_cuda() && recvbuf.is_contiguous(), "bad recvbuf");
  log_enqueue("Sendrecv", c, sendbuf.numel());
  // grouped => deadlock-free by construction
  RCCL_CHECK(ncclGroupStart());
  p2p_send(sendbuf.data_ptr(), sendbuf.numel(), nccl_dtype(sendbuf),
           sendbuf.element_size(), (int)dest, c.comm, cur_stream());
  p2p_recv(recvbuf.data_ptr(), recvbuf.numel(), nccl_dtype(recvbuf),
           recvbuf.element_size(), (int)source, c.comm, cur_stream());
  RCCL_CHECK(ncclGroupEnd());
  watchdog_arm("sendrecv", c.rank, cur_stream());
}

void barrier(int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::barrier");
  auto c = get_comm(comm_id);
  log_enqueue("Barrier", c, 1);
  // tiny allreduce on persistent scratch = a cross-rank stream barrier
  // 
  RCCL_CHECK(ncclAllReduce(c.barrier_buf, c.barrier_buf, 1, ncclInt32,
                           ncclSum, c.comm, cur_stream()));
  watchdog_arm("barrier", c.rank, cur_stream());
}

// scan: ring chain with on-device combine.
// rank r: recv running prefix from r-1, combine with own contribution on
// the CDNA4 kernel, forward to r+1.  All stream-ordered; the host never
// blocks.
void scan(at::Tensor out, at::Tensor in, int64_t op, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::scan");
  auto c = get_comm(comm_id);
  check_pair(out, in);
  auto dt = nccl_dtype(in);
  hipStream_t stream = cur_stream();
  if (c.rank == 0) {
    HIP_CHECK(hipMemcpyAsync(out.data_ptr(), in.data_ptr(),
                             in.numel() * in.element_size(),
                             hipMemcpyDeviceToDevice, stream));
  } else {
    // receive the prefix of ranks [0, r) into out, then out = out (+) in
    p2p_recv(out.data_ptr(), out.numel(), dt, out.element_size(),
             c.rank - 1, c.comm, stream);
    launch_combine(out.data_ptr(), out.data_ptr(), in.data_ptr(),
                   in.numel(), dt_code(in), (int)op, stream);
  }
  if (c.rank < c.size - 1) {
    p2p_send(out.data_ptr(), out.numel(), dt, out.element_size(),
             c.rank + 1, c.comm, stream);
  }
  log_enqueue("Scan", c, in.numel());
  watchdog_arm("scan", c.rank, stream);
}

void group_start() { RCCL_CHECK(ncclGroupStart()); }
void group_end() {
  RCCL_CHECK(ncclGroupEnd());
  watchdog_arm("group_end", -1, cur_stream());
}

// LDS-staged strided pack/unpack (CDNA4 kernels in kernels.hip).
// pack2d: gather a 2-D strided view into a contiguous buffer.
void pack2d(at::Tensor out, at::Tensor in) {
  TORCH_CHECK(in.is_cuda() && out.is_cuda(), "device tensors required");
  TORCH_CHECK(in.dim() == 2, "pack2d expects a 2-D view");
  TORCH_CHECK(out.is_contiguous() && out.numel() == in.numel(),
              "bad pack2d output");
  launch_pack2d(out.data_ptr(), in.data_ptr(), in.size(0), in.size(1),
                in.stride(0), in.stride(1), (int)in.element_size(),
                cur_stream());
}

// unpack2d: scatter a contiguous buffer into a 2-D strided view.
void unpack2d(at::Tensor out, at::Tensor in) {
  TORCH_CHECK(in.is_cuda() && out.is_cuda(), "device tensors required");
  TORCH_CHECK(out.dim() == 2, "unpack2d expects a 2-D view");
  TORCH_CHECK(in.is_contiguous() && out.numel() == in.numel(),
              "bad unpack2d input");
  launch_unpack2d(out.data_ptr(), in.data_ptr(), out.size(0), out.size(1),
                  out.stride(0), out.stride(1), (int)out.element_size(),
                  cur_stream());
}

// shallow-water stage launcher (stage = a SwStage id).  bufs order:
// fe, fn, q, ke, h, u, v, dnh, dnu, dnv, doh, dou, dov, h2, u2, v2
void sw_stage(int64_t stage, std::vector<at::Tensor> bufs, double dx,
              double dy, double dt, double nu, double cor_base,
              double cor_dj, double ab_a, double ab_b,
              std::vector<int64_t> flags) {
  TORCH_CHECK(bufs.size() == 16, "sw_stage expects 16 buffers");
  TORCH_CHECK(flags.size() == 7, "sw_stage expects 7 flags");
  const at::Tensor& h = bufs[4];
  TORCH_CHECK(h.is_cuda() && h.is_contiguous() && h.dim() == 2,
              "bad shallow-water state tensor");
  bool is_double = h.scalar_type() == at::kDouble;
  TORCH_CHECK(is_double || h.scalar_type() == at::kFloat,
              "shallow-water kernels support f32/f64");
  TORCH_CHECK(h.numel() < (int64_t)1 << 31,
              "shallow-water kernels index with 32-bit math; local domain "
              "must have fewer than 2^31 cells");
  SwLaunchParams p;
  void** slots[16] = {&p.fe, &p.fn, &p.q, &p.ke, &p.h, &p.u, &p.v,
                      &p.dnh, &p.dnu, &p.dnv, &p.doh, &p.dou, &p.dov,
                      &p.h2, &p.u2, &p.v2};
  for (int k = 0; k < 16; ++k) {
    *slots[k] = bufs[k].defined() && bufs[k].numel() ? bufs[k].data_ptr()
                                                     : nullptr;
  }
  p.ny = h.size(0);
  p.nx = h.size(1);
  p.dx = dx;
  p.dy = dy;
  p.dt = dt;
  p.nu = nu;
  p.cor_base = cor_base;
  p.cor_dj = cor_dj;
  p.ab_a = ab_a;
  p.ab_b = ab_b;
  p.south_open = (int)flags[0];
  p.north_open = (int)flags[1];
  p.west_open = (int)flags[2];
  p.east_open = (int)flags[3];
  p.east_wall = (int)flags[4];
  p.north_wall = (int)flags[5];
  p.x_wrap = (int)flags[6];
  const SwStageStatus rc =
      launch_sw_stage((int)stage, p, is_double ? 1 : 0, cur_stream());
  TORCH_CHECK(rc != SW_STAGE_UNKNOWN, "sw_stage: unknown stage id ", stage,
              " (see sw_stage_ids())");
  TORCH_CHECK(rc != SW_STAGE_F32_ONLY, "sw_stage: stage ", stage,
              " is float32-only, got float64 buffers");
}

// name -> id of every launchable stage, straight from the SwStage enum
py::dict sw_stage_ids() {
  py::dict d;
#define SW_STAGE_ITEM(name, value) d[#name] = (int)name;
  SW_STAGE_LIST(SW_STAGE_ITEM)
#undef SW_STAGE_ITEM
  return d;
}

// halo helpers ------------------------------------------------------------

void collect_field_ptrs(const std::vector<at::Tensor>& fields,
                        void* ptrs[3], bool& is_double, int64_t& ny,
                        int64_t& nx) {
  TORCH_CHECK(!fields.empty() && fields.size() <= 3,
              "1..3 halo fields supported");
  ny = fields[0].size(0);
  nx = fields[0].size(1);
  is_double = fields[0].scalar_type() == at::kDouble;
  for (size_t k = 0; k < fields.size(); ++k) {
    const auto& f = fields[k];
    TORCH_CHECK(f.is_cuda() && f.is_contiguous() && f.dim() == 2 &&
                    f.size(0) == ny && f.size(1) == nx &&
                    f.scalar_type() == fields[0].scalar_type(),
                "bad halo field");
    ptrs[k] = f.data_ptr();
  }
}

// side 0: east halo col <- col 1; side 1: west halo col <- col nx-2
void halo_wrap(std::vector<at::Tensor> fields, int64_t side) {
  void* ptrs[3];
  bool is_double;
  int64_t ny, nx;
  collect_field_ptrs(fields, ptrs, is_double, ny, nx);
  launch_halo_wrap(ptrs, (int)fields.size(), ny, nx, (int)side,
                   is_double ? 1 : 0, cur_stream());
}

void pack_cols(at::Tensor buf, std::vector<at::Tensor> fields,
               int64_t col) {
  void* ptrs[3];
  bool is_double;
  int64_t ny, nx;
  collect_field_ptrs(fields, ptrs, is_double, ny, nx);
  TORCH_CHECK(buf.is_cuda() && buf.is_contiguous() &&
                  buf.numel() >= (int64_t)fields.size() * ny,
              "bad pack buffer");
  launch_pack_cols(buf.data_ptr(), ptrs, (int)fields.size(), ny, nx, col,
                   is_double ? 1 : 0, cur_stream());
}

void unpack_cols(std::vector<at::Tensor> fields, at::Tensor buf,
                 int64_t col) {
  void* ptrs[3];
  bool is_double;
  int64_t ny, nx;
  collect_field_ptrs(fields, ptrs, is_double, ny, nx);
  launch_unpack_cols(ptrs, buf.data_ptr(), (int)fields.size(), ny, nx, col,
                     is_double ? 1 : 0, cur_stream());
}

void pack_corners(at::Tensor buf, std::vector<at::Tensor> fields) {
  void* ptrs[3];
  bool is_double;
  int64_t ny, nx;
  collect_field_ptrs(fields, ptrs, is_double, ny, nx);
  TORCH_CHECK(buf.is_cuda() && buf.is_contiguous() &&
                  buf.numel() >= 4 * (int64_t)fields.size(),
              "bad corner buffer");
  launch_pack_corners(buf.data_ptr(), ptrs, (int)fields.size(), ny, nx,
                      is_double ? 1 : 0, cur_stream());
}

void unpack_corners(std::vector<at::Tensor> fields, at::Tensor buf,
                    int64_t mask) {
  void* ptrs[3];
  bool is_double;
  int64_t ny, nx;
  collect_field_ptrs(fields, ptrs, is_double, ny, nx);
  launch_unpack_corners(ptrs, buf.data_ptr(), (int)fields.size(), ny, nx,
                        (int)mask, is_double ? 1 : 0, cur_stream());
}

// direct access to the merged staging kernels (unit tests pin them
// against the single-purpose pack/unpack kernels above)
void pack_halo(std::vector<at::Tensor> fields, int64_t wrap_side,
               c10::optional<at::Tensor> cb0, int64_t c0,
               c10::optional<at::Tensor> cb1, int64_t c1,
               c10::optional<at::Tensor> cor) {
  void* ptrs[3];
  bool is_double;
  int64_t ny, nx;
  collect_field_ptrs(fields, ptrs, is_double, ny, nx);
  launch_pack_halo(ptrs, (int)fields.size(), ny, nx, (int)wrap_side,
                   cb0 ? cb0->data_ptr() : nullptr, c0,
                   cb1 ? cb1->data_ptr() : nullptr, c1,
                   cor ? cor->data_ptr() : nullptr, is_double ? 1 : 0,
                   cur_stream());
}

void unpack_halo(std::vector<at::Tensor> fields,
                 c10::optional<at::Tensor> cb0, int64_t c0,
                 c10::optional<at::Tensor> cb1, int64_t c1,
                 c10::optional<at::Tensor> cor, int64_t cor_mask) {
  void* ptrs[3];
  bool is_double;
  int64_t ny, nx;
  collect_field_ptrs(fields, ptrs, is_double, ny, nx);
  launch_unpack_halo(ptrs, (int)fields.size(), ny, nx,
                     cb0 ? cb0->data_ptr() : nullptr, c0,
                     cb1 ? cb1->data_ptr() : nullptr, c1,
                     cor ? cor->data_ptr() : nullptr, (int)cor_mask,
                     is_double ? 1 : 0, cur_stream());
}

// One-call halo-exchange executor for the fused shallow-water step.
// Executes the schedule computed by parallel/grid.halo_exchange_schedule
// on the host side once per model (models/shallow_water.py caches it);
// the wire protocol (message set + enqueue order) is byte-identical to
// the Python executor `_exchange_fields_py`, whose cross-rank matching
// is verified per topology in tests/test_shallow_water.py.  Collapses
// ~30 Python->C++ crossings per exchange into one, which is what keeps
// the non-graph multi-rank step host-bound-free under strong scaling.
//
// Flattened schedule encoding (-1 = no peer):
//   col_ops: (k, send_to, recv_from, send_col, recv_col) x n
//   row_ops: (send_to, recv_from, recv_row, send_row) x n
//   cor_ops: (d, send_to, recv_from) x n
void sw_exchange(std::vector<at::Tensor> fields,
                 std::vector<int64_t> wrap_sides,
                 std::vector<int64_t> col_ops, std::vector<int64_t> row_ops,
                 std::vector<int64_t> cor_ops, int64_t cor_mask,
                 std::vector<at::Tensor> col_bufs, at::Tensor cor_sbuf,
                 at::Tensor cor_rbuf, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::sw_exchange");
  void* ptrs[3];
  bool is_double;
  int64_t ny, nx;
  collect_field_ptrs(fields, ptrs, is_double, ny, nx);
  const int nf = (int)fields.size();
  TORCH_CHECK(col_ops.size() % 5 == 0 && row_ops.size() % 4 == 0 &&
                  cor_ops.size() % 3 == 0,
              "bad sw_exchange schedule");
  hipStream_t stream = cur_stream();

  // stage everything outbound in ONE launch: periodic wrap + up to two
  // column packs + the corner pack (launch count bounds strong scaling)
  int wrap_side = -1;
  for (int64_t side : wrap_sides) {
    wrap_side = wrap_side < 0 ? (int)side : 2;  // two entries = both sides
  }
  void* pack_cb[2] = {nullptr, nullptr};
  int64_t pack_c[2] = {0, 0};
  for (size_t i = 0; i < col_ops.size(); i += 5) {
    if (col_ops[i + 1] < 0) continue;  // no send peer
    int64_t k = col_ops[i];
    TORCH_CHECK(0 <= k && k < 2, "bad column buffer index");
    const at::Tensor& sb = col_bufs.at(2 * k);
    TORCH_CHECK(sb.is_cuda() && sb.is_contiguous() &&
                    sb.numel() >= (int64_t)nf * ny &&
                    sb.scalar_type() == fields[0].scalar_type(),
                "bad column send buffer");
    pack_cb[k] = sb.data_ptr();
    pack_c[k] = col_ops[i + 3];
  }
  void* cor_pack = nullptr;
  if (!cor_ops.empty()) {
    TORCH_CHECK(cor_sbuf.is_cuda() && cor_sbuf.is_contiguous() &&
                    cor_sbuf.numel() >= 4 * nf,
                "bad corner send buffer");
    cor_pack = cor_sbuf.data_ptr();
  }
  if (wrap_side >= 0 || pack_cb[0] || pack_cb[1] || cor_pack) {
    launch_pack_halo(ptrs, nf, ny, nx, wrap_side, pack_cb[0], pack_c[0],
                     pack_cb[1], pack_c[1], cor_pack, is_double ? 1 : 0,
                     stream);
  }
  bool any_remote = false;
  for (size_t i = 0; i < col_ops.size(); i += 5)
    any_remote |= col_ops[i + 1] >= 0 || col_ops[i + 2] >= 0;
  for (size_t i = 0; i < row_ops.size(); i += 4)
    any_remote |= row_ops[i] >= 0 || row_ops[i + 1] >= 0;
  for (size_t i = 0; i < cor_ops.size(); i += 3)
    any_remote |= cor_ops[i + 1] >= 0 || cor_ops[i + 2] >= 0;
  if (!any_remote) return;

  auto c = get_comm(comm_id);
  auto dt = nccl_dtype(fields[0]);
  const int64_t esz = fields[0].element_size();
  log_enqueue("SwExchange", c, (int64_t)nf * ny);
  RCCL_CHECK(ncclGroupStart());
  for (size_t i = 0; i < col_ops.size(); i += 5) {
    int64_t k = col_ops[i], st = col_ops[i + 1], rf = col_ops[i + 2];
    if (st >= 0) {
      p2p_send(col_bufs.at(2 * k).data_ptr(), (int64_t)nf * ny, dt, esz,
               (int)st, c.comm, stream);
    }
    if (rf >= 0) {
      const at::Tensor& rb = col_bufs.at(2 * k + 1);
      TORCH_CHECK(rb.is_cuda() && rb.is_contiguous() &&
                      rb.numel() >= (int64_t)nf * ny,
                  "bad column recv buffer");
      p2p_recv(rb.data_ptr(), (int64_t)nf * ny, dt, esz, (int)rf, c.comm,
               stream);
    }
  }
  for (size_t i = 0; i < row_ops.size(); i += 4) {
    int64_t st = row_ops[i], rf = row_ops[i + 1];
    int64_t ridx = row_ops[i + 2], sidx = row_ops[i + 3];
    TORCH_CHECK(0 <= std::min(ridx, sidx) && std::max(ridx, sidx) < ny,
                "bad row index");
    for (int f = 0; f < nf; ++f) {
      char* base = (char*)ptrs[f];
      if (st >= 0) {
        p2p_send(base + (sidx * nx + 1) * esz, nx - 2, dt, esz, (int)st,
                 c.comm, stream);
      }
      if (rf >= 0) {
        p2p_recv(base + (ridx * nx + 1) * esz, nx - 2, dt, esz, (int)rf,
                 c.comm, stream);
      }
    }
  }
  for (size_t i = 0; i < cor_ops.size(); i += 3) {
    int64_t d = cor_ops[i], st = cor_ops[i + 1], rf = cor_ops[i + 2];
    TORCH_CHECK(0 <= d && d < 4, "bad corner index");
    if (st >= 0) {
      p2p_send((char*)cor_sbuf.data_ptr() + d * nf * esz, nf, dt, esz,
               (int)st, c.comm, stream);
    }
    if (rf >= 0) {
      TORCH_CHECK(cor_rbuf.is_cuda() && cor_rbuf.is_contiguous() &&
                      cor_rbuf.numel() >= 4 * nf,
                  "bad corner recv buffer");
      p2p_recv((char*)cor_rbuf.data_ptr() + d * nf * esz, nf, dt, esz,
               (int)rf, c.comm, stream);
    }
  }
  RCCL_CHECK(ncclGroupEnd());

  // unpack receives in ONE launch ("corners win" over column corner
  // cells — the kernel skips those column cells when a corner owns them)
  void* un_cb[2] = {nullptr, nullptr};
  int64_t un_c[2] = {0, 0};
  for (size_t i = 0; i < col_ops.size(); i += 5) {
    if (col_ops[i + 2] < 0) continue;
    int64_t k = col_ops[i];
    TORCH_CHECK(0 <= k && k < 2, "bad column buffer index");
    un_cb[k] = col_bufs.at(2 * k + 1).data_ptr();
    un_c[k] = col_ops[i + 4];
  }
  if (un_cb[0] || un_cb[1] || cor_mask) {
    launch_unpack_halo(ptrs, nf, ny, nx, un_cb[0], un_c[0], un_cb[1],
                       un_c[1], cor_mask ? cor_rbuf.data_ptr() : nullptr,
                       (int)cor_mask, is_double ? 1 : 0, stream);
  }
  watchdog_arm("sw_exchange", c.rank, stream);
}

struct HaloNdPlan {
  int64_t nf, w, esz, total;
  HaloGeom g;
  bool any_remote;
  void* fptr[kHaloMaxFields];
};

// Argument checks and slot geometry shared by halo_exchange_nd and
// halo_adjoint_nd (`who` names the entry in the one message that does).
HaloNdPlan halo_nd_plan(const char* who,
                        const std::vector<at::Tensor>& fields,
                        int64_t levels, int64_t ny, int64_t nx,
                        int64_t width, const std::vector<int64_t>& send_to,
                        const std::vector<int64_t>& recv_from,
                        int64_t local_mask, const at::Tensor& sbuf,
                        const at::Tensor& rbuf) {
  HaloNdPlan p{};
  const int64_t nf = (int64_t)fields.size();
  TORCH_CHECK(1 <= nf && nf <= kHaloMaxFields, "1..", kHaloMaxFields,
              " halo fields supported, got ", nf);
  TORCH_CHECK(send_to.size() == kHaloDirs && recv_from.size() == kHaloDirs,
              who, " expects 8 send and 8 recv peers");
  const int64_t w = width;
  TORCH_CHECK(w >= 1 && levels >= 1 && ny >= 3 * w && nx >= 3 * w,
              "bad halo geometry: levels ", levels, ", ny ", ny, ", nx ", nx,
              ", width ", w, " (each axis needs n >= 3*width)");
  TORCH_CHECK(levels < ((int64_t)1 << 31) && ny < ((int64_t)1 << 31) &&
                  nx < ((int64_t)1 << 31),
              "halo extents must be below 2^31");
  const at::Tensor& f0 = fields[0];
  const int64_t esz = f0.element_size();
  TORCH_CHECK(esz == 1 || esz == 2 || esz == 4 || esz == 8,
              "halo exchange supports 1/2/4/8-byte elements, got ", esz);
  TORCH_CHECK(levels <= f0.numel() && f0.numel() / levels == ny * nx &&
                  f0.numel() % levels == 0,
              "halo field has ", f0.numel(), " elements, expected ", levels,
              " x ", ny, " x ", nx);
  for (int64_t k = 0; k < nf; ++k) {
    const auto& f = fields[k];
    TORCH_CHECK(f.is_cuda() && f.is_contiguous() &&
                    f.numel() == f0.numel() &&
                    f.scalar_type() == f0.scalar_type() &&
                    f.device() == f0.device(),
                "bad halo field ", k);
    p.fptr[k] = f.data_ptr();
  }

  // slot geometry: [0] columns W/E, [2] rows N/S, [4] corners
  p.g = halo_geometry(nf, levels, ny, nx, w);
  const int64_t total = p.g.total;
  TORCH_CHECK(total < ((int64_t)1 << 31),
              "halo staging of ", total, " elements exceeds 2^31");
  for (const at::Tensor* b : {&sbuf, &rbuf}) {
    TORCH_CHECK(b->is_cuda() && b->is_contiguous() &&
                    b->device() == f0.device() &&
                    b->element_size() == esz && b->numel() >= total,
                "bad halo staging buffer (need ", total, " elements of ",
                esz, " bytes on the fields' device)");
  }
  TORCH_CHECK(0 <= local_mask && local_mask < (1 << kHaloDirs),
              "bad halo local mask");

  for (int i = 0; i < kHaloDirs; ++i) {
    TORCH_CHECK(send_to[i] >= -1 && recv_from[i] >= -1, "bad halo peer");
    if ((local_mask >> i) & 1) {
      TORCH_CHECK(send_to[i] >= 0 && recv_from[i] >= 0,
                  "local halo entry ", i, " needs both peers");
    } else {
      p.any_remote |= send_to[i] >= 0 || recv_from[i] >= 0;
    }
  }
  p.nf = nf;
  p.w = w;
  p.esz = esz;
  p.total = total;
  return p;
}

// Native executor of parallel/halo.HaloExchanger: one pack launch, one
// RCCL group, one unpack launch, for `levels` x (ny, nx) fields with a
// `width`-cell halo.  Entry i of send_to / recv_from (-1 = no peer) is
// direction i of halo.DIRECTIONS: W, E, N, S, then the diagonals
// (-1,-1), (-1,1), (1,-1), (1,1) as (dy, dx).  The strip sent toward
// direction d is the interior strip next to edge d; the strip received
// from -d lands in the halo at edge -d.  Column strips are full height,
// row strips cover the interior columns, corner blocks are width x width.
// Slot i of both staging buffers holds message i as
// [field][level][row][col]; slot offsets are fixed by the geometry alone,
// and computed identically by halo.py's Python executor.  Bit i of
// local_mask marks a self-peer entry: it is packed straight into slot i
// of the RECEIVE buffer and never enters the group.  Messages travel as
// raw bytes, so any dtype of a supported element size is exchanged.
//
// halo_exchange_send is the part halo_stencil_nd shares: the pack launch
// and the RCCL group.  The caller enqueues what consumes the receive slots
// (halo_exchange_nd its unpack launch, built here as `un`; halo_stencil_nd
// its own kernel) and arms the watchdog when `rank` >= 0.

// The communicator of a call with a remote entry, its peers checked
// against the communicator's size.  False when nothing is remote.
bool halo_peers(const HaloNdPlan& plan, int64_t comm_id,
                const std::vector<int64_t>& send_to,
                const std::vector<int64_t>& recv_from, CommEntry* c) {
  if (!plan.any_remote) return false;
  *c = get_comm(comm_id);
  for (int i = 0; i < kHaloDirs; ++i) {
    TORCH_CHECK(send_to[i] < c->size && recv_from[i] < c->size,
                "halo peer out of range for communicator of size ", c->size);
  }
  return true;
}

struct HaloNdSent {
  HaloNdArgs un;  // the unpack launch of this exchange
  hipStream_t stream;
  int rank;  // of this process in the group's communicator; -1: no group
};

HaloNdSent halo_exchange_send(const char* log_name, const HaloNdPlan& plan,
                              int64_t levels, int64_t ny, int64_t nx,
                              const std::vector<int64_t>& send_to,
                              const std::vector<int64_t>& recv_from,
                              int64_t local_mask, const at::Tensor& sbuf,
                              const at::Tensor& rbuf, int64_t comm_id) {
  const int64_t nf = plan.nf, w = plan.w, esz = plan.esz;
  const int64_t total = plan.total;
  const int64_t* slot_off = plan.g.slot_off;
  const int64_t *sy = plan.g.sy, *sx = plan.g.sx, *ry = plan.g.ry,
                *rx = plan.g.rx, *hh = plan.g.hh, *ww = plan.g.ww;
  auto is_local = [&](int i) { return (local_mask >> i) & 1; };
  HaloNdArgs pk{}, un{};
  for (int64_t k = 0; k < nf; ++k) pk.f[k] = un.f[k] = plan.fptr[k];

  char* sb = (char*)sbuf.data_ptr();
  char* rb = (char*)rbuf.data_ptr();
  auto fill_common = [&](HaloNdArgs& a) {
    a.ny = ny;
    a.nx = nx;
    a.levels = (unsigned)levels;
    a.nf = (int)nf;
    a.w = (int)w;
  };
  fill_common(pk);
  fill_common(un);
  auto add_seg = [&](HaloNdArgs& a, int& n, unsigned& pos, int i, char* base,
                     int64_t y0, int64_t x0) {
    HaloNdSeg& s = a.seg[n++];
    s.buf = base + slot_off[i] * esz;
    s.y0 = y0;
    s.x0 = x0;
    s.h = (unsigned)hh[i];
    s.wd = (unsigned)ww[i];
    s.start = pos;
    pos += (unsigned)(slot_off[i + 1] - slot_off[i]);
    s.end = pos;
    s.skip_lo = s.skip_hi = 0;
  };
  int npk = 0, nun = 0;
  unsigned pk_pos = 0, un_pos = 0;
  for (int i = 0; i < kHaloDirs; ++i) {
    if (send_to[i] >= 0) {
      add_seg(pk, npk, pk_pos, i, is_local(i) ? rb : sb, sy[i], sx[i]);
    }
    if (recv_from[i] >= 0) {
      add_seg(un, nun, un_pos, i, rb, ry[i], rx[i]);
      if (i < 2) {
        // column strip with x-direction dx: its low rows [0, w) are the
        // receive block of diagonal (+1, dx), its high rows of (-1, dx);
        // a present corner segment owns them ("corners win")
        const int lo = i == 0 ? 6 : 7, hi = i == 0 ? 4 : 5;
        un.seg[nun - 1].skip_lo = recv_from[lo] >= 0;
        un.seg[nun - 1].skip_hi = recv_from[hi] >= 0;
      }
    }
  }
  pk.total = pk_pos;
  un.total = un_pos;
  for (int i = npk; i < kHaloDirs; ++i) pk.seg[i].end = pk.total;
  for (int i = nun; i < kHaloDirs; ++i) un.seg[i].end = un.total;

  CommEntry c{};
  const bool remote = halo_peers(plan, comm_id, send_to, recv_from, &c);
  hipStream_t stream = cur_stream();
  launch_halo_nd(pk, 0, (int)esz, stream);
  if (remote) {
    log_enqueue(log_name, c, total);
    RCCL_CHECK(ncclGroupStart());
    for (int i = 0; i < kHaloDirs; ++i) {
      if (is_local(i)) continue;
      const int64_t nbytes = (slot_off[i + 1] - slot_off[i]) * esz;
      if (send_to[i] >= 0) {
        p2p_send(sb + slot_off[i] * esz, nbytes, ncclUint8, 1,
                 (int)send_to[i], c.comm, stream);
      }
      if (recv_from[i] >= 0) {
        p2p_recv(rb + slot_off[i] * esz, nbytes, ncclUint8, 1,
                 (int)recv_from[i], c.comm, stream);
      }
    }
    RCCL_CHECK(ncclGroupEnd());
  }
  return HaloNdSent{un, stream, remote ? c.rank : -1};
}

void halo_exchange_nd(std::vector<at::Tensor> fields, int64_t levels,
                      int64_t ny, int64_t nx, int64_t width,
                      std::vector<int64_t> send_to,
                      std::vector<int64_t> recv_from, int64_t local_mask,
                      at::Tensor sbuf, at::Tensor rbuf, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::halo_exchange_nd");
  const HaloNdPlan plan =
      halo_nd_plan("halo_exchange_nd", fields, levels, ny, nx, width,
                   send_to, recv_from, local_mask, sbuf, rbuf);
  const HaloNdSent sent =
      halo_exchange_send("HaloExchangeNd", plan, levels, ny, nx, send_to,
                         recv_from, local_mask, sbuf, rbuf, comm_id);
  launch_halo_nd(sent.un, 1, (int)plan.esz, sent.stream);
  if (sent.rank >= 0) watchdog_arm("halo_exchange_nd", sent.rank, sent.stream);
}

// The checks halo_adjoint_nd adds to halo_nd_plan's, shared with
// halo_stencil_adjoint_nd, which must pass them before its first launch.
HaloFrame halo_adjoint_checks(const HaloNdPlan& plan,
                              const std::vector<at::Tensor>& fields,
                              int64_t levels, int64_t ny, int64_t nx,
                              const at::Tensor& sbuf,
                              const at::Tensor& rbuf) {
  const auto st = fields[0].scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kDouble || st == at::kHalf ||
                  st == at::kBFloat16,
              "halo adjoint supports float16, bfloat16, float32 and "
              "float64, got ", st);
  TORCH_CHECK(sbuf.scalar_type() == st && rbuf.scalar_type() == st,
              "halo adjoint staging buffers must have the fields' dtype");
  const HaloFrame fr = halo_frame(ny, nx, plan.w);
  const int64_t work = plan.nf * levels * fr.per_level;
  TORCH_CHECK_VALUE(work < ((int64_t)1 << 31), "halo adjoint over ", work,
                    " frame cells exceeds the 2^31 work-item limit");
  return fr;
}

// Adjoint of halo_exchange_nd, in place on the gradients `fields`; same
// arguments, same slots, the schedule run backwards.  The forward pass is
// a gather (every output cell reads one input cell), so the adjoint is a
// scatter-add:
//   1. pack: the RECEIVE window of every entry with a receiver goes into
//      slot i; the rows of a column slot that a present corner entry
//      owned in the forward pass carry zeros;
//   2. one RCCL group with the peers' roles swapped: slot i is sent to
//      recv_from[i] and received from send_to[i], in the same entry
//      order, so message i still pairs with message i.  A local entry is
//      packed straight into the receive staging slot.  No group when
//      nothing is remote;
//   3. accumulate (halo_adjoint_acc_kernel): every receive window with a
//      receiver is zeroed and received slot i is added into the SEND
//      window of entry i.  Send windows overlap, so the kernel works per
//      field cell and gathers that cell's terms, last entry first.
// Floating dtypes only: step 3 is arithmetic.
void halo_adjoint_nd(std::vector<at::Tensor> fields, int64_t levels,
                     int64_t ny, int64_t nx, int64_t width,
                     std::vector<int64_t> send_to,
                     std::vector<int64_t> recv_from, int64_t local_mask,
                     at::Tensor sbuf, at::Tensor rbuf, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::halo_adjoint_nd");
  const HaloNdPlan plan =
      halo_nd_plan("halo_adjoint_nd", fields, levels, ny, nx, width,
                   send_to, recv_from, local_mask, sbuf, rbuf);
  const int64_t nf = plan.nf, w = plan.w, esz = plan.esz;
  const HaloGeom& g = plan.g;
  const HaloFrame fr =
      halo_adjoint_checks(plan, fields, levels, ny, nx, sbuf, rbuf);
  const int64_t work = nf * levels * fr.per_level;
  auto is_local = [&](int i) { return (local_mask >> i) & 1; };

  char* sb = (char*)sbuf.data_ptr();
  char* rb = (char*)rbuf.data_ptr();
  HaloNdArgs pk{};
  HaloAdjArgs ac{};
  for (int64_t k = 0; k < nf; ++k) pk.f[k] = ac.f[k] = plan.fptr[k];
  pk.ny = ac.ny = ny;
  pk.nx = ac.nx = nx;
  pk.levels = ac.levels = (unsigned)levels;
  pk.nf = ac.nf = (int)nf;
  pk.w = ac.w = (int)w;
  int npk = 0;
  unsigned pos = 0;
  for (int i = 0; i < kHaloDirs; ++i) {
    const int64_t n = g.slot_off[i + 1] - g.slot_off[i];
    if (recv_from[i] >= 0) {
      HaloNdSeg& s = pk.seg[npk++];
      s.buf = (is_local(i) ? rb : sb) + g.slot_off[i] * esz;
      s.y0 = g.ry[i];
      s.x0 = g.rx[i];
      s.h = (unsigned)g.hh[i];
      s.wd = (unsigned)g.ww[i];
      s.start = pos;
      pos += (unsigned)n;
      s.end = pos;
      s.skip_lo = s.skip_hi = 0;
      if (i < 2) {  // as in halo_exchange_nd's unpack: corners won
        const int lo = i == 0 ? 6 : 7, hi = i == 0 ? 4 : 5;
        s.skip_lo = recv_from[lo] >= 0;
        s.skip_hi = recv_from[hi] >= 0;
      }
    }
    HaloAdjSeg& a = ac.seg[i];
    a.buf = rb + g.slot_off[i] * esz;
    a.sy = (int)g.sy[i];
    a.sx = (int)g.sx[i];
    a.ry = (int)g.ry[i];
    a.rx = (int)g.rx[i];
    a.h = (unsigned)g.hh[i];
    a.wd = (unsigned)g.ww[i];
    a.acc = send_to[i] >= 0;
    a.zero = recv_from[i] >= 0;
  }
  pk.total = pos;
  for (int i = npk; i < kHaloDirs; ++i) pk.seg[i].end = pk.total;
  ac.full = fr.full;
  ac.band = fr.full ? 0u : (unsigned)fr.band;  // 2 * band <= per_level
  ac.per_level = (unsigned)fr.per_level;
  ac.total = (unsigned)work;

  CommEntry c{};
  const bool remote = halo_peers(plan, comm_id, send_to, recv_from, &c);
  hipStream_t stream = cur_stream();
  launch_halo_nd(pk, 2, (int)esz, stream);

  if (remote) {
    log_enqueue("HaloAdjointNd", c, plan.total);
    RCCL_CHECK(ncclGroupStart());
    for (int i = 0; i < kHaloDirs; ++i) {
      if (is_local(i)) continue;
      const int64_t nbytes = (g.slot_off[i + 1] - g.slot_off[i]) * esz;
      if (recv_from[i] >= 0) {
        p2p_send(sb + g.slot_off[i] * esz, nbytes, ncclUint8, 1,
                 (int)recv_from[i], c.comm, stream);
      }
      if (send_to[i] >= 0) {
        p2p_recv(rb + g.slot_off[i] * esz, nbytes, ncclUint8, 1,
                 (int)send_to[i], c.comm, stream);
      }
    }
    RCCL_CHECK(ncclGroupEnd());
    launch_halo_adjoint_acc(ac, dt_code(fields[0]), stream);
    watchdog_arm("halo_adjoint_nd", c.rank, stream);
  } else {
    launch_halo_adjoint_acc(ac, dt_code(fields[0]), stream);
  }
}

// ---- fused halo stencil (parallel/stencil.HaloStencil, stencil.hip)

// Checks of both stencil entries beyond halo_nd_plan's on `fields`, and
// the kernel arguments that do not depend on the mode.  Raises before
// anything is enqueued.
HaloStencilArgs halo_stencil_args(const char* who, const HaloNdPlan& plan,
                                  const std::vector<at::Tensor>& fields,
                                  const std::vector<at::Tensor>& outs,
                                  int64_t levels, int64_t ny, int64_t nx,
                                  const std::vector<int64_t>& tap_dy,
                                  const std::vector<int64_t>& tap_dx,
                                  const std::vector<double>& tap_coef,
                                  bool transposed, unsigned* blocks) {
  const int64_t nf = plan.nf, w = plan.w;
  TORCH_CHECK(w <= kStencilMaxWidth, who, ": stencil width ", w,
              " exceeds ", kStencilMaxWidth);
  const size_t nt = tap_dy.size();
  TORCH_CHECK(nt >= 1 && nt <= (size_t)kStencilMaxTaps &&
                  tap_dx.size() == nt && tap_coef.size() == nt,
              who, ": the three tap lists must have one length in 1..",
              kStencilMaxTaps);
  for (size_t t = 0; t < nt; ++t) {
    TORCH_CHECK(-w <= tap_dy[t] && tap_dy[t] <= w && -w <= tap_dx[t] &&
                    tap_dx[t] <= w,
                who, ": tap ", t, " reaches past the halo width ", w);
  }
  const at::Tensor& f0 = fields[0];
  const auto st = f0.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kDouble || st == at::kHalf ||
                  st == at::kBFloat16,
              who, " supports float16, bfloat16, float32 and float64, got ",
              st);
  TORCH_CHECK((int64_t)outs.size() == nf, who, ": ", nf, " field(s) but ",
              outs.size(), " output(s)");
  for (int64_t k = 0; k < nf; ++k) {
    const auto& o = outs[k];
    TORCH_CHECK(o.is_cuda() && o.is_contiguous() &&
                    o.sizes() == fields[k].sizes() &&
                    o.scalar_type() == st && o.device() == f0.device(),
                who, ": bad output ", k);
  }
  // address ranges: an output overlaps neither an input nor another output
  const int64_t bytes = f0.numel() * plan.esz;
  for (int64_t k = 0; k < nf; ++k) {
    const char* o = (const char*)outs[k].data_ptr();
    for (int64_t j = 0; j < nf; ++j) {
      const char* i = (const char*)fields[j].data_ptr();
      TORCH_CHECK_VALUE(o + bytes <= i || i + bytes <= o, who, ": output ",
                        k, " overlaps input ", j);
      if (j < k) {
        const char* p = (const char*)outs[j].data_ptr();
        TORCH_CHECK_VALUE(o + bytes <= p || p + bytes <= o, who,
                          ": output ", k, " overlaps output ", j);
      }
    }
  }
  const int64_t org = transposed ? 0 : w;
  const int64_t tiles_y = (ny - 2 * org + kStencilTileY - 1) / kStencilTileY;
  const int64_t tiles_x = (nx - 2 * org + kStencilTileX - 1) / kStencilTileX;
  // HIP refuses a launch of 2^32 threads or more: 256-thread blocks, so
  // fewer than 2^24 of them
  const int64_t planes = nf * levels;  // < 2^34
  const int64_t max_blocks = ((int64_t)1 << 32) / kStencilBlock;
  TORCH_CHECK_VALUE(tiles_y * tiles_x < max_blocks &&
                        planes * (tiles_y * tiles_x) < max_blocks,
                    who, ": ", planes, " planes of ", tiles_y, " x ", tiles_x,
                    " tiles exceed the launch limit of 2^24 blocks");
  *blocks = (unsigned)(planes * tiles_y * tiles_x);

  HaloStencilArgs a{};
  for (int64_t k = 0; k < nf; ++k) {
    a.in[k] = fields[k].data_ptr();
    a.out[k] = outs[k].data_ptr();
  }
  const int64_t stride = kStencilTileX + 2 * w;
  for (size_t t = 0; t < nt; ++t) {
    if (st == at::kDouble) {
      a.coef.f64[t] = tap_coef[t];
    } else {
      a.coef.f32[t] = (float)tap_coef[t];
    }
    const int64_t off = tap_dy[t] * stride + tap_dx[t];
    a.tap_off[t] = (int)(transposed ? -off : off);
  }
  a.ny = ny;
  a.nx = nx;
  a.levels = (unsigned)levels;
  a.tiles_y = (unsigned)tiles_y;
  a.tiles_x = (unsigned)tiles_x;
  a.w = (int)w;
  a.ntaps = (int)nt;
  return a;
}

// Native executor of HaloStencil.apply: outs = P_int . S . E (fields),
// the fields themselves never written.  Arguments as halo_exchange_nd,
// plus the outputs and the taps (dy, dx, coefficient) in the order they
// are added.
//
// Where the exchange would have written halo cell (y, x) from, by region
// (low halo, interior, high halo) along y and x: a side region from its
// column or row entry, a corner region from its corner entry or else from
// the column entry on its side ("corners win"), and from itself when that
// entry has no sender.
//   * No remote entry (direct path): ONE launch.  A received cell is read
//     from the input field at the entry's send window, so the staging
//     buffers are not touched and no communicator is looked up.
//   * Otherwise (staged path): halo_exchange_nd's pack launch and RCCL
//     group, then ONE stencil launch that reads received cells from the
//     receive slots instead of unpacking them.
// The region table of mode 0: where each of the nine regions of a plane
// reads its cells from (see above).
void halo_stencil_regions(HaloStencilArgs& a, const HaloNdPlan& plan,
                          const std::vector<int64_t>& recv_from,
                          const at::Tensor& rbuf, int64_t nx) {
  const HaloGeom& g = plan.g;
  const char* rb = (const char*)rbuf.data_ptr();
  // entry of region [ky][kx]; for a corner, the corner entry and then the
  // column entry that covers it
  static const int first[9] = {7, 2, 6, 1, -1, 0, 5, 3, 4};
  static const int second[9] = {1, -1, 0, -1, -1, -1, 1, -1, 0};
  for (int k = 0; k < 9; ++k) {
    StencilRegion& r = a.reg[k];
    r.kind = STENCIL_OWN;
    int e = first[k];
    if (e >= 0 && recv_from[e] < 0) e = second[k];
    if (e < 0 || recv_from[e] < 0) continue;
    if (plan.any_remote) {
      r.kind = STENCIL_SLOT;
      r.buf = rb + g.slot_off[e] * plan.esz;
      r.ry = (int)g.ry[e];
      r.rx = (int)g.rx[e];
      r.h = (unsigned)g.hh[e];
      r.wd = (unsigned)g.ww[e];
    } else {
      r.kind = STENCIL_OFFSET;
      r.shift = (g.sy[e] - g.ry[e]) * nx + (g.sx[e] - g.rx[e]);
    }
  }
}

void halo_stencil_nd(std::vector<at::Tensor> fields,
                     std::vector<at::Tensor> outs, int64_t levels,
                     int64_t ny, int64_t nx, int64_t width,
                     std::vector<int64_t> tap_dy,
                     std::vector<int64_t> tap_dx,
                     std::vector<double> tap_coef,
                     std::vector<int64_t> send_to,
                     std::vector<int64_t> recv_from, int64_t local_mask,
                     at::Tensor sbuf, at::Tensor rbuf, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::halo_stencil_nd");
  const char* who = "halo_stencil_nd";
  const HaloNdPlan plan = halo_nd_plan(who, fields, levels, ny, nx, width,
                                       send_to, recv_from, local_mask, sbuf,
                                       rbuf);
  unsigned blocks = 0;
  HaloStencilArgs a =
      halo_stencil_args(who, plan, fields, outs, levels, ny, nx, tap_dy,
                        tap_dx, tap_coef, false, &blocks);
  halo_stencil_regions(a, plan, recv_from, rbuf, nx);

  const int dt = dt_code(fields[0]);
  if (!plan.any_remote) {
    HIP_CHECK(launch_halo_stencil(a, 0, dt, blocks, cur_stream()));
    return;
  }
  const HaloNdSent sent =
      halo_exchange_send("HaloStencilNd", plan, levels, ny, nx, send_to,
                         recv_from, local_mask, sbuf, rbuf, comm_id);
  HIP_CHECK(launch_halo_stencil(a, 0, dt, blocks, sent.stream));
  watchdog_arm(who, sent.rank, sent.stream);
}

// ---- Krylov layer over the stencil (parallel/cg.StencilCG, krylov.hip)

// A float64 device scalar (0-d or one element) on `dev`.
double* krylov_scalar(const char* who, const char* name,
                      const at::Tensor& t, const at::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev &&
                  t.scalar_type() == at::kDouble && t.numel() == 1 &&
                  t.dim() <= 1,
              who, ": ", name,
              " must be a float64 0-d or one-element tensor on the fields' "
              "device");
  return (double*)t.data_ptr();
}

// The partials buffer: float64, contiguous, on `dev`, one slot per block.
double* krylov_partials(const char* who, const at::Tensor& t,
                        const at::Device& dev, unsigned blocks) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev &&
                  t.scalar_type() == at::kDouble && t.is_contiguous() &&
                  t.numel() >= (int64_t)blocks,
              who, ": partials must be a contiguous float64 tensor of at "
              "least ", blocks, " elements on the fields' device");
  return (double*)t.data_ptr();
}

// Neither scalar nor partials may lie inside a field that is written.
void krylov_no_overlap(const char* who, const at::Tensor& small,
                       const char* name,
                       const std::vector<at::Tensor>& written) {
  const char* lo = (const char*)small.data_ptr();
  const char* hi = lo + small.numel() * small.element_size();
  for (size_t k = 0; k < written.size(); ++k) {
    const char* f = (const char*)written[k].data_ptr();
    const char* fe = f + written[k].numel() * written[k].element_size();
    TORCH_CHECK_VALUE(hi <= f || fe <= lo, who, ": ", name,
                      " overlaps written field ", k);
  }
}

// Geometry and field checks of the elementwise Krylov entries; `lists`
// are the field lists, all of one length, shape, dtype and device.
KrylovArgs krylov_args(const char* who,
                       const std::vector<const std::vector<at::Tensor>*>&
                           lists,
                       int64_t levels, int64_t ny, int64_t nx, int64_t w,
                       bool cg, unsigned* blocks) {
  const int64_t nf = (int64_t)lists[0]->size();
  TORCH_CHECK(1 <= nf && nf <= kHaloMaxFields, who, ": 1..", kHaloMaxFields,
              " fields supported, got ", nf);
  TORCH_CHECK(w >= 1 && w <= kStencilMaxWidth && levels >= 1 &&
                  ny >= 3 * w && nx >= 3 * w,
              who, ": bad geometry: levels ", levels, ", ny ", ny, ", nx ",
              nx, ", width ", w, " (width in 1..", kStencilMaxWidth,
              ", each axis n >= 3*width)");
  TORCH_CHECK(levels < ((int64_t)1 << 31) && ny < ((int64_t)1 << 31) &&
                  nx < ((int64_t)1 << 31),
              who, ": extents must be below 2^31");
  const at::Tensor& f0 = (*lists[0])[0];
  const auto st = f0.scalar_type();
  if (cg) {
    TORCH_CHECK(st == at::kFloat || st == at::kDouble, who,
                " supports float32 and float64, got ", st);
  } else {
    TORCH_CHECK(st == at::kFloat || st == at::kDouble || st == at::kHalf ||
                    st == at::kBFloat16,
                who, " supports float16, bfloat16, float32 and float64, "
                "got ", st);
  }
  TORCH_CHECK(f0.is_cuda(), who, ": fields must live on the GPU");
  TORCH_CHECK(levels <= f0.numel() && f0.numel() % levels == 0 &&
                  f0.numel() / levels == ny * nx,
              who, ": field has ", f0.numel(), " elements, expected ",
              levels, " x ", ny, " x ", nx);
  for (size_t li = 0; li < lists.size(); ++li) {
    TORCH_CHECK((int64_t)lists[li]->size() == nf, who, ": field list ", li,
                " has ", lists[li]->size(), " field(s), expected ", nf);
    for (int64_t k = 0; k < nf; ++k) {
      const auto& f = (*lists[li])[k];
      TORCH_CHECK(f.is_cuda() && f.is_contiguous() &&
                      f.numel() == f0.numel() && f.scalar_type() == st &&
                      f.device() == f0.device(),
                  who, ": bad field ", k, " of list ", li);
    }
  }
  const int64_t tiles_y = (ny - 2 * w + kStencilTileY - 1) / kStencilTileY;
  const int64_t tiles_x = (nx - 2 * w + kStencilTileX - 1) / kStencilTileX;
  const int64_t planes = nf * levels;
  const int64_t max_blocks = ((int64_t)1 << 32) / kStencilBlock;
  TORCH_CHECK_VALUE(tiles_y * tiles_x < max_blocks &&
                        planes * (tiles_y * tiles_x) < max_blocks,
                    who, ": ", planes, " planes of ", tiles_y, " x ", tiles_x,
                    " tiles exceed the launch limit of 2^24 blocks");
  *blocks = (unsigned)(planes * tiles_y * tiles_x);
  KrylovArgs a{};
  a.ny = ny;
  a.nx = nx;
  a.levels = (unsigned)levels;
  a.tiles_y = (unsigned)tiles_y;
  a.tiles_x = (unsigned)tiles_x;
  a.w = (int)w;
  return a;
}

// `written` fields overlap neither each other nor a field of `read`
// (a field may appear in several read lists: r . r is dot(r, r)).
void krylov_fields_disjoint(const char* who,
                            const std::vector<at::Tensor>& written,
                            const std::vector<at::Tensor>& read) {
  for (size_t k = 0; k < written.size(); ++k) {
    const char* o = (const char*)written[k].data_ptr();
    const char* oe = o + written[k].numel() * written[k].element_size();
    for (size_t j = 0; j < read.size(); ++j) {
      const char* i = (const char*)read[j].data_ptr();
      const char* ie = i + read[j].numel() * read[j].element_size();
      TORCH_CHECK_VALUE(oe <= i || ie <= o, who, ": written field ", k,
                        " overlaps read field ", j);
    }
    for (size_t j = 0; j < k; ++j) {
      const char* i = (const char*)written[j].data_ptr();
      const char* ie = i + written[j].numel() * written[j].element_size();
      TORCH_CHECK_VALUE(oe <= i || ie <= o, who, ": written field ", k,
                        " overlaps written field ", j);
    }
  }
}

// HaloStencil.apply_dot: halo_stencil_nd with the kernel's DOT epilogue,
// then the finish launch: result = fields . outs over the interior of
// this rank, in float64.  Same paths, same stored outputs.
void halo_stencil_dot_nd(std::vector<at::Tensor> fields,
                         std::vector<at::Tensor> outs, int64_t levels,
                         int64_t ny, int64_t nx, int64_t width,
                         std::vector<int64_t> tap_dy,
                         std::vector<int64_t> tap_dx,
                         std::vector<double> tap_coef,
                         std::vector<int64_t> send_to,
                         std::vector<int64_t> recv_from, int64_t local_mask,
                         at::Tensor sbuf, at::Tensor rbuf, int64_t comm_id,
                         at::Tensor partials, at::Tensor result) {
  ROCTX_SCOPE("mpi4jax_amd::halo_stencil_dot_nd");
  const char* who = "halo_stencil_dot_nd";
  const HaloNdPlan plan = halo_nd_plan(who, fields, levels, ny, nx, width,
                                       send_to, recv_from, local_mask, sbuf,
                                       rbuf);
  unsigned blocks = 0;
  HaloStencilArgs a =
      halo_stencil_args(who, plan, fields, outs, levels, ny, nx, tap_dy,
                        tap_dx, tap_coef, false, &blocks);
  const at::Device dev = fields[0].device();
  a.partials = krylov_partials(who, partials, dev, blocks);
  double* res = krylov_scalar(who, "result", result, dev);
  krylov_no_overlap(who, partials, "partials", outs);
  krylov_no_overlap(who, result, "result", outs);
  krylov_no_overlap(who, result, "result", {partials});
  halo_stencil_regions(a, plan, recv_from, rbuf, nx);
  CommEntry c{};  // looked up only to be checked before the first launch
  halo_peers(plan, comm_id, send_to, recv_from, &c);

  const int dt = dt_code(fields[0]);
  if (!plan.any_remote) {
    hipStream_t stream = cur_stream();
    HIP_CHECK(launch_halo_stencil_dot(a, dt, blocks, stream));
    HIP_CHECK(launch_krylov_finish(a.partials, blocks, res, nullptr, stream));
    return;
  }
  const HaloNdSent sent =
      halo_exchange_send("HaloStencilDotNd", plan, levels, ny, nx, send_to,
                         recv_from, local_mask, sbuf, rbuf, comm_id);
  HIP_CHECK(launch_halo_stencil_dot(a, dt, blocks, sent.stream));
  HIP_CHECK(
      launch_krylov_finish(a.partials, blocks, res, nullptr, sent.stream));
  watchdog_arm(who, sent.rank, sent.stream);
}

// One Chebyshev iteration of parallel/chebyshev.StencilChebyshev on the
// interior: q = A d_in, x += d_in, r -= q, d_out = c1 * d_in + c2 * r, the
// stencil kernel's CHEB epilogue (HaloChebArgs in kernels.h).  Paths as
// halo_stencil_dot_nd: one launch with no remote peer, else the
// exchanger's pack of d_in, the RCCL group and the fused launch reading
// the receive slots.  No inner product, no scalar on the device: c1 and
// c2 travel by value.  float32 and float64 only.
void halo_cheb_step_nd(std::vector<at::Tensor> d_in,
                       std::vector<at::Tensor> d_out,
                       std::vector<at::Tensor> x, std::vector<at::Tensor> r,
                       int64_t levels, int64_t ny, int64_t nx, int64_t width,
                       std::vector<int64_t> tap_dy,
                       std::vector<int64_t> tap_dx,
                       std::vector<double> tap_coef,
                       std::vector<int64_t> send_to,
                       std::vector<int64_t> recv_from, int64_t local_mask,
                       at::Tensor sbuf, at::Tensor rbuf, int64_t comm_id,
                       double c1, double c2) {
  ROCTX_SCOPE("mpi4jax_amd::halo_cheb_step_nd");
  const char* who = "halo_cheb_step_nd";
  const HaloNdPlan plan = halo_nd_plan(who, d_in, levels, ny, nx, width,
                                       send_to, recv_from, local_mask, sbuf,
                                       rbuf);
  const auto st = d_in[0].scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kDouble, who,
              " supports float32 and float64, got ", st);
  unsigned blocks = 0;
  HaloChebArgs a{};
  static_cast<HaloStencilArgs&>(a) =
      halo_stencil_args(who, plan, d_in, d_out, levels, ny, nx, tap_dy,
                        tap_dx, tap_coef, false, &blocks);
  const std::vector<at::Tensor>* lists[2] = {&x, &r};
  for (int li = 0; li < 2; ++li) {
    TORCH_CHECK((int64_t)lists[li]->size() == plan.nf, who, ": ", plan.nf,
                " field(s) but ", lists[li]->size(), li ? " of r" : " of x");
    for (int64_t k = 0; k < plan.nf; ++k) {
      const auto& f = (*lists[li])[k];
      TORCH_CHECK(f.is_cuda() && f.is_contiguous() &&
                      f.sizes() == d_in[k].sizes() &&
                      f.scalar_type() == st &&
                      f.device() == d_in[0].device(),
                  who, ": bad field ", k, li ? " of r" : " of x");
    }
  }
  // d_in, d_out, x and r pairwise disjoint over all fields
  std::vector<at::Tensor> written(d_out);
  written.insert(written.end(), x.begin(), x.end());
  written.insert(written.end(), r.begin(), r.end());
  krylov_fields_disjoint(who, written, d_in);
  krylov_no_overlap(who, sbuf, "the send staging buffer", written);
  krylov_no_overlap(who, rbuf, "the receive staging buffer", written);
  TORCH_CHECK_VALUE(std::isfinite(c1) && std::isfinite(c2), who,
                    ": c1 and c2 must be finite, got ", c1, " and ", c2);
  for (int64_t k = 0; k < plan.nf; ++k) {
    a.x[k] = x[k].data_ptr();
    a.r[k] = r[k].data_ptr();
  }
  a.c1 = c1;
  a.c2 = c2;
  halo_stencil_regions(a, plan, recv_from, rbuf, nx);
  CommEntry c{};  // looked up only to be checked before the first launch
  halo_peers(plan, comm_id, send_to, recv_from, &c);

  const int dt = dt_code(d_in[0]);
  if (!plan.any_remote) {
    HIP_CHECK(launch_halo_stencil_cheb(a, dt, blocks, cur_stream()));
    return;
  }
  const HaloNdSent sent =
      halo_exchange_send("HaloChebStepNd", plan, levels, ny, nx, send_to,
                         recv_from, local_mask, sbuf, rbuf, comm_id);
  HIP_CHECK(launch_halo_stencil_cheb(a, dt, blocks, sent.stream));
  watchdog_arm(who, sent.rank, sent.stream);
}

// HaloStencil.dot: result = a . b over the interior of this rank.  a and
// b may be the same tensors.
void halo_interior_dot_nd(std::vector<at::Tensor> a_fields,
                          std::vector<at::Tensor> b_fields, int64_t levels,
                          int64_t ny, int64_t nx, int64_t width,
                          at::Tensor partials, at::Tensor result) {
  ROCTX_SCOPE("mpi4jax_amd::halo_interior_dot_nd");
  const char* who = "halo_interior_dot_nd";
  unsigned blocks = 0;
  KrylovArgs a = krylov_args(who, {&a_fields, &b_fields}, levels, ny, nx,
                             width, false, &blocks);
  const at::Device dev = a_fields[0].device();
  a.partials = krylov_partials(who, partials, dev, blocks);
  double* res = krylov_scalar(who, "result", result, dev);
  krylov_no_overlap(who, result, "result", {partials});
  for (size_t k = 0; k < a_fields.size(); ++k) {
    a.a[k] = a_fields[k].data_ptr();
    a.b[k] = b_fields[k].data_ptr();
  }
  hipStream_t stream = cur_stream();
  HIP_CHECK(launch_krylov(a, KRYLOV_DOT, dt_code(a_fields[0]), blocks,
                          stream));
  HIP_CHECK(launch_krylov_finish(a.partials, blocks, res, nullptr, stream));
}

// One CG update on the interior: alpha = rs / pq (0 when pq == 0),
// x += alpha p, r -= alpha q; then the finish launch stores the old rs in
// rs_old and this rank's r . r, on the stored r, in rs.
void halo_cg_update_nd(std::vector<at::Tensor> x, std::vector<at::Tensor> r,
                       std::vector<at::Tensor> p, std::vector<at::Tensor> q,
                       int64_t levels, int64_t ny, int64_t nx, int64_t width,
                       at::Tensor rs, at::Tensor pq, at::Tensor rs_old,
                       at::Tensor partials) {
  ROCTX_SCOPE("mpi4jax_amd::halo_cg_update_nd");
  const char* who = "halo_cg_update_nd";
  unsigned blocks = 0;
  KrylovArgs a =
      krylov_args(who, {&x, &r, &p, &q}, levels, ny, nx, width, true,
                  &blocks);
  const at::Device dev = x[0].device();
  a.partials = krylov_partials(who, partials, dev, blocks);
  a.num = krylov_scalar(who, "rs", rs, dev);
  a.den = krylov_scalar(who, "pq", pq, dev);
  double* old = krylov_scalar(who, "rs_old", rs_old, dev);
  std::vector<at::Tensor> written(x), read(p);
  written.insert(written.end(), r.begin(), r.end());
  read.insert(read.end(), q.begin(), q.end());
  krylov_fields_disjoint(who, written, read);
  const at::Tensor* small[4] = {&rs, &pq, &rs_old, &partials};
  const char* names[4] = {"rs", "pq", "rs_old", "partials"};
  for (int i = 0; i < 4; ++i) {
    krylov_no_overlap(who, *small[i], names[i], written);
    for (int j = 0; j < i; ++j) {
      krylov_no_overlap(who, *small[i], names[i], {*small[j]});
    }
  }
  for (size_t k = 0; k < x.size(); ++k) {
    a.a[k] = p[k].data_ptr();
    a.b[k] = q[k].data_ptr();
    a.x[k] = x[k].data_ptr();
    a.r[k] = r[k].data_ptr();
  }
  hipStream_t stream = cur_stream();
  HIP_CHECK(launch_krylov(a, KRYLOV_UPDATE, dt_code(x[0]), blocks, stream));
  HIP_CHECK(launch_krylov_finish(a.partials, blocks, (double*)a.num, old,
                                 stream));
}

// The CG direction on the interior: beta = rs / rs_old (0 when
// rs_old == 0), p = r + beta p.  The halo of p is not written.
void halo_cg_direction_nd(std::vector<at::Tensor> p,
                          std::vector<at::Tensor> r, int64_t levels,
                          int64_t ny, int64_t nx, int64_t width,
                          at::Tensor rs, at::Tensor rs_old) {
  ROCTX_SCOPE("mpi4jax_amd::halo_cg_direction_nd");
  const char* who = "halo_cg_direction_nd";
  unsigned blocks = 0;
  KrylovArgs a =
      krylov_args(who, {&p, &r}, levels, ny, nx, width, true, &blocks);
  const at::Device dev = p[0].device();
  a.num = krylov_scalar(who, "rs", rs, dev);
  a.den = krylov_scalar(who, "rs_old", rs_old, dev);
  krylov_fields_disjoint(who, p, r);
  krylov_no_overlap(who, rs, "rs", p);
  krylov_no_overlap(who, rs_old, "rs_old", p);
  for (size_t k = 0; k < p.size(); ++k) {
    a.a[k] = r[k].data_ptr();
    a.r[k] = p[k].data_ptr();
  }
  HIP_CHECK(launch_krylov(a, KRYLOV_DIRECTION, dt_code(p[0]), blocks,
                          cur_stream()));
}

// Native executor of HaloStencil.adjoint: gins = E^T . S^T . P_int (gouts).
// One launch of the stencil kernel's transposed mode writes every cell of
// `gins`; halo_adjoint_nd then runs in place on them.
void halo_stencil_adjoint_nd(std::vector<at::Tensor> gouts,
                             std::vector<at::Tensor> gins, int64_t levels,
                             int64_t ny, int64_t nx, int64_t width,
                             std::vector<int64_t> tap_dy,
                             std::vector<int64_t> tap_dx,
                             std::vector<double> tap_coef,
                             std::vector<int64_t> send_to,
                             std::vector<int64_t> recv_from,
                             int64_t local_mask, at::Tensor sbuf,
                             at::Tensor rbuf, int64_t comm_id) {
  ROCTX_SCOPE("mpi4jax_amd::halo_stencil_adjoint_nd");
  const char* who = "halo_stencil_adjoint_nd";
  const HaloNdPlan plan = halo_nd_plan(who, gouts, levels, ny, nx, width,
                                       send_to, recv_from, local_mask, sbuf,
                                       rbuf);
  unsigned blocks = 0;
  const HaloStencilArgs a =
      halo_stencil_args(who, plan, gouts, gins, levels, ny, nx, tap_dy,
                        tap_dx, tap_coef, true, &blocks);
  // everything halo_adjoint_nd will ask of `gins`, before the launch
  halo_adjoint_checks(plan, gouts, levels, ny, nx, sbuf, rbuf);
  CommEntry c{};  // looked up only to be checked before the launch
  halo_peers(plan, comm_id, send_to, recv_from, &c);

  HIP_CHECK(launch_halo_stencil(a, 1, dt_code(gouts[0]), blocks,
                                cur_stream()));
  halo_adjoint_nd(std::move(gins), levels, ny, nx, width, std::move(send_to),
                  std::move(recv_from), local_mask, std::move(sbuf),
                  std::move(rbuf), comm_id);
}

// direct access to the combine kernel (used by gpu numerics tests)
void combine(at::Tensor dst, at::Tensor a, at::Tensor b, int64_t op) {
  check_pair(dst, a);
  check_pair(dst, b);
  launch_combine(dst.data_ptr(), a.data_ptr(), b.data_ptr(), a.numel(),
                 dt_code(a), (int)op, cur_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "mpi4jax_amd native RCCL/HIP bridge (gfx950)";
  m.def("get_unique_id", &get_unique_id);
  m.def("comm_init_rank", &comm_init_rank);
  m.def("comm_destroy", &comm_destroy);
  m.def("destroy_all_comms", &destroy_all_comms);
  m.def("comm_count", &comm_count);
  m.def("check_async_errors", &check_async_errors);
  m.def("comm_abort", &comm_abort);
  m.def("comm_register", &comm_register);
  m.def("comm_deregister", &comm_deregister);
  m.def("set_logging", &set_logging);
  m.def("set_watchdog", &set_watchdog);
  m.def("get_watchdog", &get_watchdog);
  m.def("debug_wedge_stream", &debug_wedge_stream);
  m.def("version_info", &version_info);
  m.def("build_info", &build_info);
  m.def("allreduce", &allreduce);
  m.def("reduce", &reduce);
  m.def("allgather", &allgather);
  m.def("broadcast", &broadcast);
  m.def("reduce_scatter", &reduce_scatter);
  m.def("alltoall", &alltoall);
  m.def("gather", &gather);
  m.def("scatter", &scatter);
  m.def("send", &send);
  m.def("recv", &recv);
  m.def("sendrecv", &sendrecv);
  m.def("barrier", &barrier);
  m.def("scan", &scan);
  m.def("group_start", &group_start);
  m.def("group_end", &group_end);
  m.def("pack2d", &pack2d);
  m.def("unpack2d", &unpack2d);
  m.def("combine", &combine);
  m.def("sw_stage", &sw_stage);
  m.def("sw_stage_ids", &sw_stage_ids);
  m.def("halo_wrap", &halo_wrap);
  m.def("pack_cols", &pack_cols);
  m.def("unpack_cols", &unpack_cols);
  m.def("pack_corners", &pack_corners);
  m.def("unpack_corners", &unpack_corners);
  m.def("sw_exchange", &sw_exchange);
  m.def("pack_halo", &pack_halo);
  m.def("unpack_halo", &unpack_halo);
  m.def("halo_exchange_nd", &halo_exchange_nd);
  m.def("halo_adjoint_nd", &halo_adjoint_nd);
  m.def("halo_stencil_nd", &halo_stencil_nd);
  m.def("halo_stencil_adjoint_nd", &halo_stencil_adjoint_nd);
  m.def("halo_stencil_dot_nd", &halo_stencil_dot_nd);
  m.def("halo_cheb_step_nd", &halo_cheb_step_nd);
  m.def("halo_interior_dot_nd", &halo_interior_dot_nd);
  m.def("halo_cg_update_nd", &halo_cg_update_nd);
  m.def("halo_cg_direction_nd", &halo_cg_direction_nd);
}
