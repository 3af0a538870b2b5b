#include "CompressorSet.h"

#include <cstdio>
#include <cstdlib>

#include "DeviceCompressor.h"
#include "TraceFile.h"
#include "mpc_hip.h"

namespace comp
{

CompressorSet::CompressorSet(const std::vector<Compressor *> &members) : m_Members(members), m_Group(nullptr)
{
  std::vector<mpc_handle *> handles;
  for (size_t i = 0; i < m_Members.size(); i++) {
    mpc_handle *h = m_Members[i] ? m_Members[i]->DeviceHandle() : nullptr;
    if (!h) {
      printf("CompressorSet: member %zu%s%s is not a GPU evaluator (VPC, BDI, FPC, BPC, SC2, Pattern, CPACK): it cannot be fed in a set.\n", i,
             m_Members[i] ? " " : "", m_Members[i] ? m_Members[i]->GetCompressorName().c_str() : "");
      exit(1);
    }
    handles.push_back(h);
  }
  int rc = mpc_group_create(handles.data(), handles.size(), &m_Group);
  if (rc != MPC_OK) fail("CompressorSet: cannot create the group", rc, mpc_group_last_error(nullptr));
}

CompressorSet::~CompressorSet() { mpc_group_destroy(m_Group); }

std::string CompressorSet::GetForm() const { return mpc_group_form(m_Group); }

void CompressorSet::Prepare()
{
  for (Compressor *c : m_Members) (void)c->DeviceHandle();
}

void CompressorSet::CompressBatch(const uint8_t *lines, unsigned long long n)
{
  Prepare();
  int rc = mpc_group_compress_batch(m_Group, lines, n, nullptr, nullptr);
  if (rc != MPC_OK) fail("CompressorSet::CompressBatch", rc, mpc_group_last_error(m_Group));
}

void CompressorSet::EnableBest()
{
  Prepare();
  int rc = mpc_group_best_enable(m_Group);
  if (rc != MPC_OK) fail("CompressorSet::EnableBest", rc, mpc_group_last_error(m_Group));
}

BestReport CompressorSet::GetBest(unsigned sectorBytes)
{
  Prepare();
  BestReport best(GetLineSize());
  best.Sizes.SectorBytes = sectorBytes;
  best.Sizes.Bins.assign(MPC_SIZE_BINS, 0);
  best.Wins.assign(m_Members.size(), 0);
  uint64_t bits = 0, lines = 0;
  int rc = mpc_group_best_get(m_Group, best.Sizes.Bins.data(), best.Sizes.Bins.size(), best.Wins.data(), best.Wins.size(), &bits, &lines);
  if (rc != MPC_OK) fail("CompressorSet::GetBest", rc, mpc_group_last_error(m_Group));
  best.BestBits = bits;
  best.Lines = lines;
  size_t takingPart = 0;
  for (Compressor *c : m_Members) {
    mpc_info info;
    takingPart += mpc_get_info(c->DeviceHandle(), &info) == MPC_OK && info.algorithm != 5;      // (5: Pattern)
  }
  while ((1ull << best.TagBits) < takingPart) best.TagBits++;
  return best;
}

void CompressorSet::EnableClassStats(unsigned sectorBytes)
{
  Prepare();
  int rc = mpc_group_class_stats_enable(m_Group, sectorBytes);
  if (rc != MPC_OK) fail("CompressorSet::EnableClassStats", rc, mpc_group_last_error(m_Group));
  m_ClassSectorBytes = sectorBytes;
}

ClassReport CompressorSet::GetClassStats(size_t i)
{
  Prepare();
  ClassReport report(GetLineSize(), m_ClassSectorBytes);
  report.Table.assign(MPC_CLASS_TABLE_LEN, 0);
  int rc = mpc_group_class_stats_get(m_Group, i == BestMember ? MPC_CLASS_BEST : (int)i, report.Table.data(), report.Table.size());
  if (rc != MPC_OK) fail("CompressorSet::GetClassStats", rc, mpc_group_last_error(m_Group));
  return report;
}

void CompressorSet::EnablePackStats(unsigned long long blockLines, unsigned sectorBytes, unsigned headerBits)
{
  Prepare();
  int rc = mpc_group_pack_stats_enable(m_Group, blockLines, sectorBytes, headerBits);
  if (rc != MPC_OK) fail("CompressorSet::EnablePackStats", rc, mpc_group_last_error(m_Group));
}

PackReport CompressorSet::GetPackStats(size_t i)
{
  Prepare();
  PackReport report(GetLineSize());
  int rc = mpc_group_pack_stats_get(m_Group, i == BestMember ? MPC_PACK_BEST : (int)i, report.Table.data(), report.Table.size());
  if (rc != MPC_OK) fail("CompressorSet::GetPackStats", rc, mpc_group_last_error(m_Group));
  return report;
}

void CompressorSet::EnableImageStats(unsigned long long blockLines, unsigned sectorBytes, unsigned headerBits, unsigned long long capacityLines)
{
  Prepare();
  int rc = mpc_group_image_stats_enable(m_Group, capacityLines, blockLines, sectorBytes, headerBits);
  if (rc != MPC_OK) fail("CompressorSet::EnableImageStats", rc, mpc_group_last_error(m_Group));
}

ImageReport CompressorSet::GetImageStats(size_t i)
{
  Prepare();
  ImageReport report(GetLineSize());
  int rc = mpc_group_image_stats_get(m_Group, (int)i, report.Table.data(), report.Table.size());
  if (rc != MPC_OK) fail("CompressorSet::GetImageStats", rc, mpc_group_last_error(m_Group));
  return report;
}

void CompressorSet::EnableRewriteStats(unsigned granuleBytes, unsigned long long capacityLines)
{
  Prepare();
  int rc = mpc_group_rewrite_stats_enable(m_Group, capacityLines, granuleBytes);
  if (rc != MPC_OK) fail("CompressorSet::EnableRewriteStats", rc, mpc_group_last_error(m_Group));
}

RewriteReport CompressorSet::GetRewriteStats(size_t i)
{
  Prepare();
  RewriteReport report(GetLineSize());
  int rc = mpc_group_rewrite_stats_get(m_Group, (int)i, report.Table.data(), report.Table.size());
  if (rc != MPC_OK) fail("CompressorSet::GetRewriteStats", rc, mpc_group_last_error(m_Group));
  return report;
}

void CompressorSet::SetLogClassField(int field)
{
  int rc = mpc_group_class_log_field(m_Group, field);
  if (rc != MPC_OK) fail("CompressorSet::SetLogClassField", rc, mpc_group_last_error(m_Group));
}

void CompressorSet::ClassFromMember(size_t i)
{
  int rc = mpc_group_class_from_member(m_Group, (int)i);
  if (rc != MPC_OK) fail("CompressorSet::ClassFromMember", rc, mpc_group_last_error(m_Group));
}

unsigned long long CompressorSet::CompressFile(const std::string &tracePath)
{
  Prepare();
  uint64_t done = 0;
  int rc = trace::IsGpgpuSimLog(tracePath) ? mpc_group_compress_gpgpusim_log(m_Group, tracePath.c_str(), nullptr, &done)
                                           : mpc_group_compress_npy(m_Group, tracePath.c_str(), 0, ~0ull, 1, &done);
  if (rc != MPC_OK) fail("CompressorSet::CompressFile", rc, mpc_group_last_error(m_Group));
  return done;
}

}  // namespace comp
