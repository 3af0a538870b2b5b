// Compressor.cpp -- default of the additive comp::Compressor::CompressFile(): the reference driver's own loop
// (src/main.cpp:208-248) over a loader chosen by the file's extension (main.cpp:74-84), for evaluators that only
// implement CompressLine().  The GPU evaluators override it with a streamed batch path.
#include "Compressor.h"

#include <cstdio>
#include <cstdlib>

#include "TraceFile.h"

namespace comp
{

unsigned long long Compressor::CompressFile(const std::string &tracePath)
{
  trace::MemReq_t *memReq = nullptr;
  trace::Loader *loader = trace::OpenByExtension(tracePath, GetLineSize(), &memReq);
  if (!loader) {
    printf("Invalid File! %s\n", tracePath.c_str());
    exit(1);
  }
  const unsigned long long done = trace::CompressPerLine(this, loader, memReq);
  delete memReq;
  delete loader;
  return done;
}

}  // namespace comp
