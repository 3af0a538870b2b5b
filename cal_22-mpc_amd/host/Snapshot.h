// Snapshot.h -- ADDITIVE, no counterpart in the reference: the memory image of a GPGPU-Sim .log trace as data (mpc_snapshot,
// include/mpc_hip_snapshot.h).  Per distinct unit address the bytes of the latest request there; Evaluate feeds the
// address-aligned lines of lineSize = 1, 2, 4 or 8 units, in ascending address order, to an evaluator or a set, which
// count them like any other lines: with their addresses when image accounting is on there.
#ifndef MPC_HOST_SNAPSHOT_H
#define MPC_HOST_SNAPSHOT_H

#include <string>

#include "CompressorSet.h"
#include "DeviceCompressor.h"
#include "SnapshotReport.h"

struct mpc_snapshot;

namespace comp
{

class Snapshot
{
public:
  // unitBytes: 32, 64 or 128; capacityUnits: the distinct unit addresses it can hold.  A failure exits with a message, as
  // the evaluators' constructors do.
  explicit Snapshot(unsigned unitBytes, unsigned long long capacityUnits = 1ull << 24);
  ~Snapshot();
  Snapshot(const Snapshot &) = delete;
  Snapshot &operator=(const Snapshot &) = delete;

  // Needs no device: whether a snapshot of these values can write lines of lineSize bytes (mpc_snapshot_check_values);
  // false with the library's message in `why`
  static bool CheckValues(unsigned unitBytes, unsigned long long capacityUnits, unsigned lineSize, std::string &why);
  unsigned GetUnitBytes() const { return m_UnitBytes; }
  // every evaluated record of the .log at its mem_addr, in file order; returns the units added
  unsigned long long AddFile(const std::string &logPath);
  // the emitted lines of (lineSize, zeroFill) to the evaluator or to every member of the set; returns their number
  unsigned long long Evaluate(DeviceCompressor &compressor, unsigned lineSize, bool zeroFill = false, bool byPresence = false);
  unsigned long long Evaluate(CompressorSet &set, unsigned lineSize, bool zeroFill = false, bool byPresence = false);
  SnapshotReport GetReport(unsigned lineSize, bool zeroFill = false);

private:
  [[noreturn]] void Fail(const std::string &what, int rc);
  mpc_snapshot *m_Snapshot;
  unsigned m_UnitBytes;
};

}  // namespace comp

#endif
