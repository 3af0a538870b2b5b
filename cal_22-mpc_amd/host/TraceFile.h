// TraceFile.h -- the decisions about a trace file that the driver (main.cpp), the default Compressor::CompressFile()
// and the GPU evaluators share: which loader reads it (reference main.cpp:74-84), whether the library streams it as
// a GPGPU-Sim .log, and the reference driver's per-line loop (main.cpp:208-248).  Inline: needs the loaders and utils.cpp only.
#ifndef MPC_HOST_TRACEFILE_H
#define MPC_HOST_TRACEFILE_H

#include <string>

#include "Compressor.h"
#include "LoaderAPSim.h"
#include "LoaderGPGPU.h"
#include "LoaderNPY.h"
#include "utils.h"

namespace trace
{

// What a GPU evaluator's CompressFile() hands to the library's .log reader; every other path goes to its .npy reader.
inline bool IsGpgpuSimLog(const std::string &path) { return path.size() > 4 && mpctext::ends_with(path, ".log"); }

// The loader for the file's extension and, in *memReq, the request object its GetCacheline() takes; the caller deletes
// both.  apsimLineSize: the line size asked of the APSim loader.  nullptr (and no request) for any other extension.
inline Loader *OpenByExtension(const std::string &path, unsigned apsimLineSize, MemReq_t **memReq)
{
  if (mpctext::ends_with(path, ".npy")) {
    *memReq = new MemReq_t;
    return new LoaderNPY(path);
  }
  if (mpctext::ends_with(path, ".log")) {
    *memReq = new gpgpusim::MemReqGPU_t;
    return new gpgpusim::LoaderGPGPU(path);
  }
  if (mpctext::ends_with(path, ".txt")) {
    *memReq = new apsim::MemReqGPU_t;
    return new apsim::LoaderGPGPU(path, apsimLineSize);
  }
  *memReq = nullptr;
  return nullptr;
}

// The reference's loop: one request object handed back and forth, GetCacheline() -> isEnd? -> CompressLine(); of a
// .log trace only the GLOBAL_ACC_R / GLOBAL_ACC_W requests (main.cpp:222-224).  Returns the number of lines evaluated.
inline unsigned long long CompressPerLine(comp::Compressor *compressor, Loader *loader, MemReq_t *memReq)
{
  const bool filtered = dynamic_cast<gpgpusim::MemReqGPU_t *>(memReq) != nullptr;
  unsigned long long done = 0;
  memReq->Reset();
  while (1) {
    memReq = loader->GetCacheline(memReq);
    if (memReq->isEnd) break;
    if (filtered && !gpgpusim::LoaderGPGPU::isEvaluated(static_cast<gpgpusim::MemReqGPU_t *>(memReq)->reqType)) continue;
    compressor->CompressLine(memReq->data);
    done++;
  }
  return done;
}

}  // namespace trace

#endif
