// CompressorSet.h -- ADDITIVE, no counterpart in the reference: several GPU evaluators over one trace at the cost of
// one pass.  The reference compares compressors by running its driver once per algorithm (main.cpp:208-248 each
// time); a CompressorSet feeds every member the same lines while the trace is read and staged once (mpc_group,
// include/mpc_hip.h).  Each member keeps its own statistics: GetResult(i) is the member's GetResult(), and its
// Print() / PrintDetail() write what a run with that member alone writes.
#ifndef MPC_HOST_COMPRESSORSET_H
#define MPC_HOST_COMPRESSORSET_H

#include <string>
#include <vector>

#include "Compressor.h"
#include "ClassReport.h"
#include "ImageReport.h"
#include "PackReport.h"
#include "RewriteReport.h"
#include "SizeReport.h"

struct mpc_group;

namespace comp
{

class CompressorSet
{
public:
  // Members are borrowed and must outlive the set; every one must be a GPU evaluator (VPC, BDI, FPC, BPC, SC2, Pattern) of the
  // same line size.  Anything else is refused with a message (exit(1), as the evaluators' constructors do).
  explicit CompressorSet(const std::vector<Compressor *> &members);
  ~CompressorSet();
  CompressorSet(const CompressorSet &) = delete;
  CompressorSet &operator=(const CompressorSet &) = delete;

  size_t Size() const { return m_Members.size(); }
  unsigned GetLineSize() { return m_Members[0]->GetLineSize(); }
  // which members share a kernel launch, e.g. "VPC: unrolled; BDI+FPC+BPC: one kernel"
  std::string GetForm() const;

  // n consecutive lines of GetLineSize() bytes to every member
  void CompressBatch(const uint8_t *lines, unsigned long long n);
  // a .npy file (all rows but the last, as the reference driver does) or a GPGPU-Sim .log file to every member;
  // returns the number of lines evaluated
  unsigned long long CompressFile(const std::string &tracePath);
  CompResult *GetResult(size_t i) { return m_Members[i]->GetResult(); }
  // ADDITIVE: account, from now on, the per-line smallest size over the members (mpc_group_best_enable: every member
  // but Pattern ones, ties to the first minimal member); refused with a message when fewer than two take part
  void EnableBest();
  BestReport GetBest(unsigned sectorBytes = ACCESS_GRAN);
  // ADDITIVE: per-class sums for every member and, with EnableBest (before or after), for the per-line smallest size
  // (mpc_group_class_stats_enable); off by default
  void EnableClassStats(unsigned sectorBytes = ACCESS_GRAN);
  // member i's sums, or with i == BestMember those of the best-of
  static constexpr size_t BestMember = (size_t)-1;
  ClassReport GetClassStats(size_t i);
  void SetLogClassField(int field);
  // the class of a line is member i's selected + 1: a VPC member's cluster + 1, 0 = uncompressed (mpc_group_class_from_member)
  void ClassFromMember(size_t i);
  // ADDITIVE: EnablePackStats for every member with the same values; after EnableBest also a table of the per-line smallest
  // size, counted with headerBits + blockLines x tag bits (mpc_group_pack_stats_enable); off by default
  void EnablePackStats(unsigned long long blockLines, unsigned sectorBytes = ACCESS_GRAN, unsigned headerBits = 0);
  // member i's table, or with i == BestMember that of the per-line smallest size
  PackReport GetPackStats(size_t i);
  // ADDITIVE: EnableImageStats for every member with the same values; a member's image is its own
  // (mpc_group_image_stats_enable); off by default
  void EnableImageStats(unsigned long long blockLines, unsigned sectorBytes = ACCESS_GRAN, unsigned headerBits = 0,
                        unsigned long long capacityLines = 1ull << 24);
  // member i's table
  ImageReport GetImageStats(size_t i);
  // ADDITIVE: EnableRewriteStats for every member with the same values; a member's map is its own
  // (mpc_group_rewrite_stats_enable); off by default
  void EnableRewriteStats(unsigned granuleBytes = ACCESS_GRAN, unsigned long long capacityLines = 1ull << 24);
  // member i's table
  RewriteReport GetRewriteStats(size_t i);
  // ADDITIVE: the group itself, for what feeds it from the device (Snapshot::Evaluate); the members' buffered lines go
  // first and every member counts as fed
  mpc_group *DeviceGroup() { Prepare(); return m_Group; }

private:
  void Prepare();      // members' buffered lines first
  std::vector<Compressor *> m_Members;
  mpc_group *m_Group;
  unsigned m_ClassSectorBytes = 0;
};

}  // namespace comp

#endif
