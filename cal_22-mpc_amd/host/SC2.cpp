#include "SC2.h"

#include <cstdio>
#include <cstdlib>

#include "mpc_hip.h"

namespace comp
{

static void fail(const char *what, int rc, mpc_handle *h)
{
  const char *msg = mpc_last_error(h);
  printf("%s (%d): %s\n", what, rc, msg ? msg : "");
  exit(1);
}

SC2::SC2(unsigned lineSize, unsigned warmupCnt) : m_Handle(nullptr), m_LineSize(lineSize), m_Started(false)
{
  int rc = mpc_create_sc2(lineSize, warmupCnt, -1, &m_Handle);
  if (rc != MPC_OK) fail("SC2: cannot create the evaluator", rc, nullptr);
  m_Stat = new CompResult(lineSize);
  m_Stat->CompressorName = "SC2-Huffman";
}

SC2::~SC2() { mpc_destroy(m_Handle); }

void SC2::SetSamplingCnt(unsigned cnt)
{
  FlushLines();
  if (m_Started) {
    printf("SC2::SetSamplingCnt after the first line is not supported (the warm-up sample has begun).\n");
    exit(1);
  }
  mpc_destroy(m_Handle);
  m_Handle = nullptr;
  int rc = mpc_create_sc2(m_LineSize, cnt, -1, &m_Handle);
  if (rc != MPC_OK) fail("SC2::SetSamplingCnt", rc, nullptr);
}

unsigned SC2::CompressLine(std::vector<uint8_t> &dataLine)
{
  if (dataLine.size() != m_LineSize) {
    printf("SC2: line of %zu bytes, expected %u.\n", dataLine.size(), m_LineSize);
    exit(1);
  }
  m_Started = true;
  if (LineBuffering()) {
    BufferLine(dataLine);
    return 0;
  }
  uint16_t bits = 0;
  int rc = mpc_compress_batch(m_Handle, dataLine.data(), 1, &bits, nullptr);
  if (rc != MPC_OK) fail("SC2::CompressLine", rc, m_Handle);
  return bits;
}

void SC2::CompressBatch(const uint8_t *lines, unsigned long long n)
{
  FlushLines();
  m_Started = m_Started || n > 0;
  int rc = mpc_compress_batch(m_Handle, lines, n, nullptr, nullptr);
  if (rc != MPC_OK) fail("SC2::CompressBatch", rc, m_Handle);
}

unsigned long long SC2::CompressFile(const std::string &tracePath)
{
  FlushLines();
  m_Started = true;
  uint64_t done = 0;
  const bool isLog = tracePath.size() > 4 && tracePath.compare(tracePath.size() - 4, 4, ".log") == 0;
  int rc = isLog ? mpc_compress_gpgpusim_log(m_Handle, tracePath.c_str(), nullptr, &done)
                 : mpc_compress_npy(m_Handle, tracePath.c_str(), 0, ~0ull, 1, &done);
  if (rc != MPC_OK) fail("SC2::CompressFile", rc, m_Handle);
  return done;
}

// CompResult only (SC2's PrintDetail is empty, SC2.h)
CompResult *SC2::GetResult()
{
  FlushLines();
  uint64_t v[6];
  int rc = mpc_stats_get(m_Handle, v, 6);
  if (rc != MPC_OK) fail("SC2::GetResult", rc, m_Handle);
  m_Stat->OriginalSize = v[1];
  m_Stat->CompressedSize = v[2];
  m_Stat->CompRatio = v[0] ? (double)v[1] / (double)v[2] : 0.0;
  return m_Stat;
}

}  // namespace comp
