#include "SnapshotReport.h"

#include <fstream>
#include <iostream>

#include "CompResult.h"

namespace comp
{

void SnapshotReport::Print(std::string workloadName, std::string filePath)
{
  std::ofstream file;
  if (filePath != "")
    CompResult::openForAppend(file, filePath,
                              "Workload,Unit Bytes,Line Size,Partial,Units,Distinct Units,Misaligned,Touched Lines,Complete Lines,Partial Lines,Missing Units,Evaluated Lines,\n");
  std::ostream &stream = (filePath == "") ? std::cout : file;
  stream << workloadName << "," << UnitBytes() << "," << LineSize << "," << (ZeroFill ? "zero" : "skip") << "," << Units() << "," << DistinctUnits() << ","
         << Misaligned() << "," << TouchedLines() << "," << CompleteLines() << "," << PartialLines() << "," << MissingUnits() << "," << EvaluatedLines()
         << "," << std::endl;
}

}  // namespace comp
