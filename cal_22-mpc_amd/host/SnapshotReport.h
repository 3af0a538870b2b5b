// SnapshotReport.h -- ADDITIVE, no counterpart in the reference: what a snapshot (Snapshot.h) held and which lines of it
// were evaluated -- the units added, the distinct ones, and at the line size of the evaluation the touched, complete and
// partial lines.  Next to ImageReport.h, which reports the sizes of an image; this one reports its shape.
#ifndef MPC_HOST_SNAPSHOTREPORT_H
#define MPC_HOST_SNAPSHOTREPORT_H

#include <cstdint>
#include <string>
#include <vector>

namespace comp
{

struct SnapshotReport {
  static constexpr size_t TableLen = 8;      // MPC_SNAPSHOT_TABLE_LEN (include/mpc_hip_snapshot.h)

  SnapshotReport(unsigned lineSize, bool zeroFill) : Stats(TableLen, 0), Plan(TableLen, 0), LineSize(lineSize), ZeroFill(zeroFill) {}

  // Appends one row to filePath (stdout for ""), the header first when the file does not exist yet, as the result
  // classes' Print does:
  //   Workload,Unit Bytes,Line Size,Partial,Units,Distinct Units,Misaligned,Touched Lines,Complete Lines,Partial Lines,Missing Units,Evaluated Lines,
  // Partial: "skip" or "zero".
  void Print(std::string workloadName = "", std::string filePath = "");

  uint64_t Units() const { return Stats[0]; }
  uint64_t DistinctUnits() const { return Stats[1]; }
  uint64_t Misaligned() const { return Stats[2]; }
  uint64_t Capacity() const { return Stats[3]; }
  unsigned UnitBytes() const { return (unsigned)Stats[4]; }
  uint64_t TouchedLines() const { return Plan[0]; }
  uint64_t CompleteLines() const { return Plan[1]; }
  uint64_t PartialLines() const { return Plan[2]; }
  uint64_t PartialUnits() const { return Plan[3]; }
  uint64_t MissingUnits() const { return Plan[4]; }
  uint64_t EvaluatedLines() const { return Plan[5]; }

  std::vector<uint64_t> Stats, Plan;     // the layouts of mpc_snapshot_stats and mpc_snapshot_plan
  unsigned LineSize;
  bool ZeroFill;
};

}  // namespace comp

#endif
