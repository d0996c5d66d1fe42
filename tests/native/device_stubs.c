/* Stand-ins for the device layer of libbfhip, for host-only harnesses that link the host sources without a GPU
 * (tests/native/plan_oom.c): every entry aborts, so a run also proves that the paths it drives never reach a device.
 * Only the public headers are included here: the stand-ins are declared without prototypes, which the declarations of
 * bfhip_internal.h would contradict. */
#include <stdio.h>
#include <stdlib.h>

#include "bfhip_build.h"

#define STUB(name) int name() { fprintf(stderr, "device layer reached: %s\n", #name); abort(); }
/* releasing nothing is fine; releasing something is not */
void bfdevFree(void *p) { if (p) { fprintf(stderr, "device layer reached: bfdevFree(non-NULL)\n"); abort(); } }
void bfdevEventDestroy(void *e) { if (e) { fprintf(stderr, "device layer reached: bfdevEventDestroy(non-NULL)\n"); abort(); } }
void bfdevHostFreePinned(void *p) { if (p) { fprintf(stderr, "device layer reached: bfdevHostFreePinned(non-NULL)\n"); abort(); } }
STUB(bfdevBuildEval)
STUB(bfdevBuildGemm)
STUB(bfdevBuildJacobi)
STUB(bfdevBuildPack)
STUB(bfdevBuildQrcp)
STUB(bfdevQrcpFits)
STUB(bfdevEventCreate)
STUB(bfdevEventElapsed)
STUB(bfdevEventRecord)
STUB(bfdevEventSync)
STUB(bfdevScalePermute)
STUB(bfdevGetDevice)
STUB(bfdevHostAllocPinned)
STUB(bfdevGmresDot)
STUB(bfdevGmresDots)
STUB(bfdevGmresDotsFinish)
STUB(bfdevGmresProject)
STUB(bfdevGmresFinish)
STUB(bfdevGmresMgsStep)
STUB(bfdevGmresResidual)
STUB(bfdevGmresUpdate)
STUB(bfdevHelm2Dense)
STUB(bfdevLaunchReduce)
STUB(bfdevLaunchFlow)
STUB(bfdevFlowGrid)
STUB(bfdevMemsetAsync)
STUB(bfdevLaunchStage)
STUB(bfdevMalloc)
STUB(bfdevMemFree)
STUB(bfdevMemcpyD2DAsync)
STUB(bfdevMemcpyD2H)
STUB(bfdevMemcpyD2HAsync)
STUB(bfdevMemcpyH2D)
STUB(bfdevMemcpyH2DAsync)
STUB(bfdevMemset)
STUB(bfdevSetDevice)
STUB(bfdevPointerKind)
STUB(bfdevMemcpyAnyAsync)
STUB(bfdevHostRegister)
STUB(bfdevHostUnregister)
STUB(bfdevSync)
STUB(bfdevSynthFill)
/* the sharded step lives in bfhip_shard.hip (device layer) */
size_t bfhipShardedGetNumRows(const BfhipSharded *sh) { (void)sh; fprintf(stderr, "device layer reached: bfhipShardedGetNumRows\n"); abort(); }
size_t bfhipShardedGetNumCols(const BfhipSharded *sh) { (void)sh; fprintf(stderr, "device layer reached: bfhipShardedGetNumCols\n"); abort(); }
STUB(bfhipShardedApplyHost)
STUB(bfhipShardedOperator)
void bfhipShardedFree(BfhipSharded **p) { if (p && *p) { fprintf(stderr, "device layer reached: bfhipShardedFree(non-NULL)\n"); abort(); } }
