/* stub_ccl.c -- an in-process stand-in for the seven RCCL entry points libbfhip.so resolves (bfhip_shard.hip: loadRccl),
 * so that the sharded C-ABI step can run with 2, 3 and 5 ranks on ONE GPU: the ranks are host threads of one process, a
 * "world" is a table entry keyed by the 128-byte unique id.  libbfhip.so loads it through BFHIP_RCCL_LIBRARY.
 *
 * Host-only C: no kernels, only HIP runtime calls (stream synchronisation and copies).
 *
 * Ordering between ranks is kept on the HOST only -- a collective never makes one stream wait on another on the device:
 *   it synchronises its own stream and publishes its pointers; meets the other ranks at a barrier; does its copies on its
 *   own stream and synchronises again; meets a second barrier before returning (a peer cannot overwrite a send slot
 *   another rank is still reading).
 * ncclAllGather: possibly in place (send == recv + rank * count): a device-to-device copy of every peer's `count`
 *   elements into slot q of this rank's receive buffer.
 * ncclAllReduce: in place, ncclSum, ncclFloat32 / ncclFloat64: every rank reads all ranks' buffers to host memory and,
 *   after a barrier, adds them IN RANK ORDER 0..W-1 IN THE BUFFER'S OWN SCALAR TYPE and writes the result back.  The order
 *   is part of the contract: every rank's result is identical (as RCCL guarantees) and reproducible in numpy.
 * Barriers are timed (20 s; STUB_CCL_DEADLINE_SECONDS overrides): a wait past the deadline, or a world marked aborted,
 *   returns an error code and does not block.  ncclCommAbort marks the world aborted and wakes the waiters.
 * Test entry points: stubCclFailNext (a rank's next collective returns an error BEFORE it meets the barrier) and
 *   stubCclCalls (calls per function per rank).  Worlds and communicators live in static tables and are never freed, so
 *   the counters of a destroyed or aborted communicator stay readable. */
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <errno.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#define STUB_MAX_RANKS 16
#define STUB_MAX_WORLDS 256

enum { STUB_GET_UNIQUE_ID = 0, STUB_COMM_INIT_RANK, STUB_COMM_DESTROY, STUB_COMM_ABORT, STUB_ALL_GATHER, STUB_ALL_REDUCE, STUB_NUM_FUNCS };

typedef struct StubWorld StubWorld;
struct ncclComm {                 /* rccl.h declares the opaque `struct ncclComm`; this is the stub's definition */
  StubWorld *world;
  int rank, live;
};

struct StubWorld {
  char id[NCCL_UNIQUE_ID_BYTES];
  int used, nranks, joined, aborted;
  pthread_mutex_t mu;
  pthread_cond_t cv;
  int waiting;                    /* ranks inside the current barrier */
  unsigned generation;
  struct ncclComm comm[STUB_MAX_RANKS];
  int failNext[STUB_MAX_RANKS];
  long calls[STUB_MAX_RANKS][STUB_NUM_FUNCS];
  /* what a rank published for the collective in flight */
  void const *send[STUB_MAX_RANKS];
  void *recv[STUB_MAX_RANKS];
  size_t count[STUB_MAX_RANKS];
  int dtype[STUB_MAX_RANKS];
};

static StubWorld worlds[STUB_MAX_WORLDS];
static pthread_mutex_t tableMu = PTHREAD_MUTEX_INITIALIZER;
static unsigned long idCounter;
static long idCalls;              /* ncclGetUniqueId has no rank */

static double deadlineSeconds(void) {
  char const *e = getenv("STUB_CCL_DEADLINE_SECONDS");
  double v = e ? atof(e) : 0;
  return v > 0 ? v : 20.0;
}

/* the world of an id; created on first sight when nranks > 0 */
static StubWorld *findWorld(void const *id, int nranks) {
  StubWorld *w = NULL;
  pthread_mutex_lock(&tableMu);
  for (int i = 0; i < STUB_MAX_WORLDS && !w; ++i)
    if (worlds[i].used && !memcmp(worlds[i].id, id, NCCL_UNIQUE_ID_BYTES)) w = &worlds[i];
  for (int i = 0; i < STUB_MAX_WORLDS && !w && nranks > 0; ++i)
    if (!worlds[i].used) {
      w = &worlds[i];
      memset(w, 0, sizeof *w);
      memcpy(w->id, id, NCCL_UNIQUE_ID_BYTES);
      pthread_mutex_init(&w->mu, NULL);
      pthread_condattr_t attr;
      pthread_condattr_init(&attr);
      pthread_condattr_setclock(&attr, CLOCK_MONOTONIC);
      pthread_cond_init(&w->cv, &attr);
      pthread_condattr_destroy(&attr);
      w->nranks = nranks;
      w->used = 1;
    }
  pthread_mutex_unlock(&tableMu);
  return w;
}

/* all ranks of the world meet here; 0, or an error code when the world is aborted or the deadline passes */
static ncclResult_t barrier(StubWorld *w) {
  struct timespec until;
  clock_gettime(CLOCK_MONOTONIC, &until);
  double const d = deadlineSeconds();
  until.tv_sec += (time_t)d;
  until.tv_nsec += (long)((d - (double)(time_t)d) * 1e9);
  if (until.tv_nsec >= 1000000000L) { until.tv_sec += 1; until.tv_nsec -= 1000000000L; }
  ncclResult_t rc = ncclSuccess;
  pthread_mutex_lock(&w->mu);
  if (w->aborted) rc = ncclInternalError;
  else if (++w->waiting == w->nranks) {
    w->waiting = 0;
    ++w->generation;
    pthread_cond_broadcast(&w->cv);
  } else {
    unsigned const gen = w->generation;
    while (gen == w->generation && !w->aborted) {
      if (pthread_cond_timedwait(&w->cv, &w->mu, &until) == ETIMEDOUT && gen == w->generation && !w->aborted) {
        w->aborted = 1;           /* a rank that never arrived: nobody waits for it again */
        pthread_cond_broadcast(&w->cv);
        rc = ncclSystemError;
      }
    }
    if (gen == w->generation) rc = rc ? rc : ncclInternalError;       /* woken by an abort, not by the last arrival */
  }
  pthread_mutex_unlock(&w->mu);
  return rc;
}

static ncclResult_t hipRc(hipError_t e) { return e == hipSuccess ? ncclSuccess : ncclUnhandledCudaError; }

/* entry of a collective: count the call, honour stubCclFailNext and a dead world, drain this rank's stream */
static ncclResult_t enter(ncclComm_t comm, int func, hipStream_t stream) {
  if (!comm || !comm->world) return ncclInvalidArgument;
  StubWorld *w = comm->world;
  int fail, aborted;
  pthread_mutex_lock(&w->mu);
  ++w->calls[comm->rank][func];
  fail = w->failNext[comm->rank];
  w->failNext[comm->rank] = 0;
  aborted = w->aborted || !comm->live;
  pthread_mutex_unlock(&w->mu);
  if (fail) return ncclSystemError;
  if (aborted) return ncclInternalError;
  return hipRc(hipStreamSynchronize(stream));
}

ncclResult_t ncclGetUniqueId(ncclUniqueId *uniqueId) {
  if (!uniqueId) return ncclInvalidArgument;
  memset(uniqueId, 0, sizeof *uniqueId);
  pthread_mutex_lock(&tableMu);
  unsigned long const serial = ++idCounter;
  ++idCalls;
  pthread_mutex_unlock(&tableMu);
  snprintf(uniqueId->internal, sizeof uniqueId->internal, "stub-ccl:%ld:%lu", (long)getpid(), serial);
  return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t *comm, int nranks, ncclUniqueId commId, int rank) {
  if (!comm || nranks < 1 || nranks > STUB_MAX_RANKS || rank < 0 || rank >= nranks) return ncclInvalidArgument;
  *comm = NULL;
  StubWorld *w = findWorld(commId.internal, nranks);
  if (!w) return ncclSystemError;
  ncclResult_t rc = ncclSuccess;
  pthread_mutex_lock(&w->mu);
  ++w->calls[rank][STUB_COMM_INIT_RANK];
  if (w->nranks != nranks || w->comm[rank].world) rc = ncclInvalidUsage;         /* another size, or the rank is taken */
  else { w->comm[rank].world = w; w->comm[rank].rank = rank; w->comm[rank].live = 1; ++w->joined; }
  pthread_mutex_unlock(&w->mu);
  if (rc) return rc;
  if ((rc = barrier(w))) return rc;                                               /* like RCCL: returns once every rank has joined */
  *comm = &w->comm[rank];
  return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  if (!comm || !comm->world) return ncclInvalidArgument;
  StubWorld *w = comm->world;
  ncclResult_t rc = ncclSuccess;
  pthread_mutex_lock(&w->mu);
  ++w->calls[comm->rank][STUB_COMM_DESTROY];
  if (!comm->live) rc = ncclInvalidArgument;                                      /* destroyed or aborted before */
  comm->live = 0;
  pthread_mutex_unlock(&w->mu);
  return rc;
}

ncclResult_t ncclCommAbort(ncclComm_t comm) {
  if (!comm || !comm->world) return ncclInvalidArgument;
  StubWorld *w = comm->world;
  pthread_mutex_lock(&w->mu);
  ++w->calls[comm->rank][STUB_COMM_ABORT];
  comm->live = 0;
  w->aborted = 1;
  pthread_cond_broadcast(&w->cv);
  pthread_mutex_unlock(&w->mu);
  return ncclSuccess;
}

static size_t scalarSize(ncclDataType_t dt) { return dt == ncclFloat32 ? 4 : dt == ncclFloat64 ? 8 : 0; }

ncclResult_t ncclAllGather(const void *sendbuff, void *recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream) {
  ncclResult_t rc = enter(comm, STUB_ALL_GATHER, stream);
  if (rc) return rc;
  size_t const es = scalarSize(datatype);
  if (!es || !sendbuff || !recvbuff) return ncclInvalidArgument;
  StubWorld *w = comm->world;
  int const me = comm->rank;
  pthread_mutex_lock(&w->mu);
  w->send[me] = sendbuff; w->recv[me] = recvbuff; w->count[me] = sendcount; w->dtype[me] = (int)datatype;
  pthread_mutex_unlock(&w->mu);
  if ((rc = barrier(w))) return rc;
  size_t const bytes = sendcount * es;
  for (int q = 0; q < w->nranks && !rc; ++q) {
    if (w->count[q] != sendcount || w->dtype[q] != (int)datatype) { rc = ncclInvalidArgument; break; }
    char *dst = (char *)recvbuff + (size_t)q * bytes;
    if (bytes && dst != (char const *)w->send[q]) rc = hipRc(hipMemcpyAsync(dst, w->send[q], bytes, hipMemcpyDeviceToDevice, stream));
  }
  if (!rc) rc = hipRc(hipStreamSynchronize(stream));
  ncclResult_t const rb = barrier(w);
  return rc ? rc : rb;
}

ncclResult_t ncclAllReduce(const void *sendbuff, void *recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm, hipStream_t stream) {
  ncclResult_t rc = enter(comm, STUB_ALL_REDUCE, stream);
  if (rc) return rc;
  size_t const es = scalarSize(datatype);
  if (!es || op != ncclSum || !sendbuff || sendbuff != recvbuff) return ncclInvalidArgument;
  StubWorld *w = comm->world;
  int const me = comm->rank, nr = w->nranks;
  pthread_mutex_lock(&w->mu);
  w->send[me] = sendbuff; w->recv[me] = recvbuff; w->count[me] = count; w->dtype[me] = (int)datatype;
  pthread_mutex_unlock(&w->mu);
  size_t const bytes = count * es;
  char *host = (char *)malloc((size_t)nr * bytes + 1);
  if (!host) { (void)ncclCommAbort(comm); return ncclSystemError; }
  if ((rc = barrier(w))) { free(host); return rc; }
  for (int q = 0; q < nr && !rc; ++q) {
    if (w->count[q] != count || w->dtype[q] != (int)datatype) { rc = ncclInvalidArgument; break; }
    if (bytes) rc = hipRc(hipMemcpyAsync(host + (size_t)q * bytes, w->send[q], bytes, hipMemcpyDeviceToHost, stream));
  }
  if (!rc) rc = hipRc(hipStreamSynchronize(stream));
  ncclResult_t const rb = barrier(w);                   /* every rank has read every buffer: they may be overwritten now */
  if (!rc) rc = rb;
  if (!rc) {
    /* rank order 0..W-1, in the scalar type of the buffer */
    if (datatype == ncclFloat32) {
      float *acc = (float *)host;
      for (int q = 1; q < nr; ++q) { float const *p = (float const *)(host + (size_t)q * bytes); for (size_t i = 0; i < count; ++i) acc[i] = acc[i] + p[i]; }
    } else {
      double *acc = (double *)host;
      for (int q = 1; q < nr; ++q) { double const *p = (double const *)(host + (size_t)q * bytes); for (size_t i = 0; i < count; ++i) acc[i] = acc[i] + p[i]; }
    }
    if (bytes) rc = hipRc(hipMemcpyAsync(recvbuff, host, bytes, hipMemcpyHostToDevice, stream));
    if (!rc) rc = hipRc(hipStreamSynchronize(stream));
  }
  free(host);
  return rc;
}

const char *ncclGetErrorString(ncclResult_t result) {
  switch (result) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "stub collective: HIP error";
    case ncclSystemError: return "stub collective: injected failure or barrier deadline";
    case ncclInternalError: return "stub collective: the world was aborted";
    case ncclInvalidArgument: return "stub collective: invalid argument";
    case ncclInvalidUsage: return "stub collective: invalid usage";
    default: return "stub collective: error";
  }
}

/* ---- test entry points ---------------------------------------------------------------------------------------------- */

/* rank's next collective (all-gather or all-reduce) in the world of `id128` returns an error before it meets the barrier */
int stubCclFailNext(void const *id128, int rank) {
  StubWorld *w = id128 ? findWorld(id128, 0) : NULL;
  if (!w || rank < 0 || rank >= w->nranks) return -1;
  pthread_mutex_lock(&w->mu);
  w->failNext[rank] = 1;
  pthread_mutex_unlock(&w->mu);
  return 0;
}

/* calls of function `func` (the STUB_* enum order: GetUniqueId, CommInitRank, CommDestroy, CommAbort, AllGather, AllReduce)
 * by `rank` in the world of `id128`; ncclGetUniqueId is counted per process; -1: unknown world / rank / function */
long stubCclCalls(void const *id128, int rank, int func) {
  if (func == STUB_GET_UNIQUE_ID) return idCalls;
  StubWorld *w = id128 ? findWorld(id128, 0) : NULL;
  if (!w || rank < 0 || rank >= w->nranks || func < 0 || func >= STUB_NUM_FUNCS) return -1;
  pthread_mutex_lock(&w->mu);
  long const n = w->calls[rank][func];
  pthread_mutex_unlock(&w->mu);
  return n;
}
