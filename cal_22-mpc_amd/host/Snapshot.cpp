#include "Snapshot.h"

#include "mpc_hip.h"

namespace comp
{

static int partialOf(bool zeroFill) { return zeroFill ? MPC_SNAPSHOT_PARTIAL_ZERO : MPC_SNAPSHOT_PARTIAL_SKIP; }

void Snapshot::Fail(const std::string &what, int rc) { fail(what, rc, mpc_snapshot_last_error(m_Snapshot)); }

Snapshot::Snapshot(unsigned unitBytes, unsigned long long capacityUnits) : m_Snapshot(nullptr), m_UnitBytes(unitBytes)
{
  int rc = mpc_snapshot_create(unitBytes, capacityUnits, -1, &m_Snapshot);
  if (rc != MPC_OK) Fail("Snapshot: cannot create the snapshot", rc);
}

bool Snapshot::CheckValues(unsigned unitBytes, unsigned long long capacityUnits, unsigned lineSize, std::string &why)
{
  if (mpc_snapshot_check_values(unitBytes, capacityUnits, lineSize) == MPC_OK) return true;
  why = mpc_snapshot_last_error(nullptr);
  return false;
}

Snapshot::~Snapshot() { mpc_snapshot_destroy(m_Snapshot); }

unsigned long long Snapshot::AddFile(const std::string &logPath)
{
  uint64_t added = 0;
  int rc = mpc_snapshot_add_gpgpusim_log(m_Snapshot, logPath.c_str(), &added);
  if (rc != MPC_OK) Fail("Snapshot::AddFile", rc);
  return added;
}

unsigned long long Snapshot::Evaluate(DeviceCompressor &compressor, unsigned lineSize, bool zeroFill, bool byPresence)
{
  int rc = mpc_snapshot_evaluate(m_Snapshot, compressor.DeviceHandle(), lineSize, partialOf(zeroFill), byPresence ? 1 : 0);
  if (rc != MPC_OK) Fail("Snapshot::Evaluate", rc);
  return GetReport(lineSize, zeroFill).EvaluatedLines();
}

unsigned long long Snapshot::Evaluate(CompressorSet &set, unsigned lineSize, bool zeroFill, bool byPresence)
{
  int rc = mpc_snapshot_evaluate_group(m_Snapshot, set.DeviceGroup(), lineSize, partialOf(zeroFill), byPresence ? 1 : 0);
  if (rc != MPC_OK) Fail("Snapshot::Evaluate", rc);
  return GetReport(lineSize, zeroFill).EvaluatedLines();
}

SnapshotReport Snapshot::GetReport(unsigned lineSize, bool zeroFill)
{
  SnapshotReport report(lineSize, zeroFill);
  int rc = mpc_snapshot_stats(m_Snapshot, report.Stats.data());
  if (rc == MPC_OK) rc = mpc_snapshot_plan(m_Snapshot, lineSize, partialOf(zeroFill), report.Plan.data());
  if (rc != MPC_OK) Fail("Snapshot::GetReport", rc);
  return report;
}

}  // namespace comp
