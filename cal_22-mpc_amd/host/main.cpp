// main.cpp -- the `compressor` command line of the reference (src/main.cpp), kept
// flag-for-flag:  compressor -a ALGO -i TRACE [-c CONFIG.json] [-o OUTDIR] [-h]
// stdout "comp.ratio: <double>", CSV rows appended to OUTDIR/<stem>_results.csv and
// OUTDIR/<stem>_results_detail.csv.  This build evaluates VPC, BDI, FPC and BPC (the hot path
// of SURVEY.md section 8) on the MI355X; traces are .npy files, GPGPU-Sim .log files
// (GLOBAL_ACC_R / GLOBAL_ACC_W requests, reference main.cpp:222-224) or APSim .txt files
// (32-byte data beats of handshaking channels).  The other algorithm names are recognised
// and reported as not part of this build.
// ADDITIVE: -a takes a comma-separated list (-a VPC,BDI,FPC,BPC): every algorithm of the list is evaluated in ONE pass
// over the trace (comp::CompressorSet) and writes exactly the files a run with its name alone writes.
// ADDITIVE: --size-histogram / --sector BYTES also write OUTDIR/<stem>_results_sizes.csv (comp::SizeReport: the
// distribution of the per-line sizes and the sectors they occupy) and, for a list, the per-line best of the list as
// BEST_results_sizes.csv and a "BEST comp.ratio:" line.  Without them nothing changes.
// ADDITIVE: --by kernel|rw|mftype|cluster also writes OUTDIR/<stem>_results_classes.csv (comp::ClassReport: lines, bits,
// ratio and sector ratio per class of a line).  kernel, rw and mftype take the class from the records of a .log trace;
// cluster takes it from the first VPC member of a list (its cluster + 1, 0 = uncompressed).  With a list every member
// gets its file, and with --size-histogram the per-line best of the list BEST_results_classes.csv.  --sector sets the
// sector size of these files too.  Without --by nothing changes.
// ADDITIVE: --pack N [--sector BYTES] [--pack-header BITS] also writes OUTDIR/<stem>_results_pack.csv (comp::PackReport: the
// sectors that blocks of N consecutive lines occupy when they are packed and rounded up once).  With a list every member
// gets its file, and with --size-histogram the per-line best of the list BEST_results_pack.csv.  Next to --pack, --sector
// does not imply --size-histogram.  Without --pack nothing changes.
// ADDITIVE: --image N [--sector BYTES] [--image-header BITS] [--image-capacity LINES] also writes
// OUTDIR/<stem>_results_image.csv (comp::ImageReport: the latest size per line address of a GPGPU-Sim .log trace's
// mem_addr, and the sectors that address-aligned blocks of N lines of that image occupy).  With a list every member gets
// its file.  It needs a .log input.  Next to --image, --sector does not imply --size-histogram.  Without --image nothing changes.
// ADDITIVE: --rewrites GRANULE [--rewrite-capacity LINES] also writes OUTDIR/<stem>_results_rewrites.csv
// (comp::RewriteReport: per line address of a GPGPU-Sim .log trace's mem_addr the sequence of sizes, as transitions
// between size classes of GRANULE bytes, with the latest and the peak granules).  With a list every member gets its file.
// It needs a .log input and is refused next to --snapshot, where every address occurs once.  Without --rewrites nothing changes.
// ADDITIVE: --snapshot L [--snapshot-partial skip|zero] [--snapshot-capacity UNITS] evaluates, instead of the requests of a
// GPGPU-Sim .log trace, the memory they touched: the latest bytes per request address (comp::Snapshot), written out as
// address-aligned lines of L bytes in ascending address order.  The usual files are written with the workload named
// <name>@snapshot<L>, and OUTDIR/<stem>_results_snapshot.csv (comp::SnapshotReport) as well.  Without --snapshot nothing changes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "BDI.h"
#include "BPC.h"
#include "CompressorSet.h"
#include "FPC.h"
#include "Snapshot.h"
#include "TraceFile.h"
#include "VPC.h"

#define REQ_SIZE 32   // line size asked of the APSim loader (reference main.cpp:23)

struct Args;
static int runList(const std::vector<std::string> &names, const std::string &tracePath, const std::string &configPath,
                   const std::string &outputDirPath, const Args &a);

static const char *kHelp =
    "Usage:\n"
    "  Compressor [OPTION...]\n"
    "\n"
    "  -a, --algorithm arg  Compression algorithm\n"
    "                       [VPC/FPC/BDI/BPC/CPACK/SC2/PATTERN/VIEWER]. Default=VPC\n"
    "                       A list (VPC,BDI,FPC,BPC) is evaluated in one pass.\n"
    "  -i, --input arg      Input GPGPU-Sim trace file path. Supported extensions:\n"
    "                       .log, .npy\n"
    "  -c, --config arg     Config file path (.json).\n"
    "  -o, --output arg     Output directory path\n"
    "      --size-histogram Also write <stem>_results_sizes.csv: lines per compressed\n"
    "                       size and per number of sectors; for a list also the\n"
    "                       per-line best of the list (BEST_results_sizes.csv)\n"
    "      --sector arg     Sector size in bytes for that file. Default=32\n"
    "                       (implies --size-histogram)\n"
    "      --pack arg       Also write <stem>_results_pack.csv: the sectors that blocks\n"
    "                       of that many consecutive lines occupy when packed; the\n"
    "                       sector size is --sector's (which then implies nothing).\n"
    "      --pack-header arg Bits added to every block of --pack. Default=0\n"
    "      --image arg      Also write <stem>_results_image.csv: the latest size per\n"
    "                       line address of a .log trace, and the sectors that aligned\n"
    "                       blocks of that many lines occupy; the sector size is\n"
    "                       --sector's (which then implies nothing).\n"
    "      --image-header arg Bits added to every block of --image. Default=0\n"
    "      --image-capacity arg Distinct lines the image can hold. Default=16777216\n"
    "      --rewrites arg   Also write <stem>_results_rewrites.csv: how the size of a\n"
    "                       line of a .log trace changes when its address comes again,\n"
    "                       in size classes of that many bytes\n"
    "      --rewrite-capacity arg Distinct lines --rewrites can follow.\n"
    "                       Default=16777216\n"
    "      --snapshot arg   Evaluate, instead of the requests of a .log trace, the\n"
    "                       memory they touched: the latest bytes per address as\n"
    "                       aligned lines of that many bytes (1, 2, 4 or 8 requests,\n"
    "                       at most 256); also writes <stem>_results_snapshot.csv\n"
    "      --snapshot-partial arg Lines with requests missing: skip them or fill\n"
    "                       the gaps with zero bytes [skip/zero]. Default=skip\n"
    "      --snapshot-capacity arg Distinct request addresses the snapshot can\n"
    "                       hold. Default=16777216\n"
    "      --by arg         Also write <stem>_results_classes.csv: lines, bits and\n"
    "                       sectors per class of a line [kernel/rw/mftype/cluster].\n"
    "                       kernel, rw, mftype: a field of a .log trace's records;\n"
    "                       cluster: the first VPC of a list picks the class\n"
    "  -h, --help           Print usage\n";

struct Args {
  std::string algorithm, input, config, output;
  bool has_algorithm = false, has_input = false, has_config = false, has_output = false, help = false;
  bool per_line = false;   // ADDITIVE --per-line: the reference's loop (GetCacheline -> CompressLine per line) instead of batches
  unsigned long long line_buffer = 0;   // ADDITIVE --line-buffer N: that loop with Compressor::SetLineBuffering(N)
  bool size_histogram = false;          // ADDITIVE --size-histogram: <stem>_results_sizes.csv (SizeReport.h)
  unsigned sector = ACCESS_GRAN;        // ADDITIVE --sector BYTES: the sector size of that file; implies --size-histogram
  std::string by;                       // ADDITIVE --by kernel|rw|mftype|cluster: <stem>_results_classes.csv (ClassReport.h); empty: off
  bool has_by = false;
  bool has_sector = false;
  bool has_pack = false, has_pack_header = false;      // ADDITIVE --pack N [--pack-header BITS]: <stem>_results_pack.csv (PackReport.h)
  unsigned long long pack = 0;
  unsigned pack_header = 0;
  bool has_image = false, has_image_header = false, has_image_capacity = false;      // ADDITIVE --image N [...]: <stem>_results_image.csv (ImageReport.h)
  unsigned long long image = 0, image_capacity = 1ull << 24;
  unsigned image_header = 0;
  bool has_rewrites = false, has_rewrite_capacity = false;      // ADDITIVE --rewrites GRANULE [--rewrite-capacity LINES]: <stem>_results_rewrites.csv (RewriteReport.h)
  unsigned long long rewrites = 0, rewrite_capacity = 1ull << 24;
  bool has_snapshot = false, has_snapshot_partial = false, has_snapshot_capacity = false;      // ADDITIVE --snapshot L [...]: Snapshot.h
  unsigned long long snapshot = 0, snapshot_capacity = 1ull << 24;
  std::string snapshot_partial = "skip";
};

// the value of --pack / --pack-header: digits only, up to `most`
static bool takeNumber(const std::string &value, unsigned long long most, unsigned long long &out)
{
  char *end = nullptr;
  out = strtoull(value.c_str(), &end, 10);
  return !value.empty() && value[0] >= '0' && value[0] <= '9' && *end == 0 && value.size() <= 19 && out <= most;
}

static bool take_value(int argc, char **argv, int &i, const std::string &arg, const char *shortf, const char *longf,
                       std::string &out, bool &seen)
{
  const std::string lf = std::string("--") + longf;
  if (arg == shortf || arg == lf) {
    if (i + 1 >= argc) {
      std::cout << "Option '" << longf << "' is missing an argument" << std::endl;
      exit(1);
    }
    out = argv[++i];
    seen = true;
    return true;
  }
  if (arg.compare(0, lf.size() + 1, lf + "=") == 0) {
    out = arg.substr(lf.size() + 1);
    seen = true;
    return true;
  }
  if (arg.size() > 2 && arg.compare(0, 2, shortf) == 0) {   // -aVPC
    out = arg.substr(2);
    seen = true;
    return true;
  }
  return false;
}

// The algorithms the reference knows and this build leaves out: one message, true when name is one of them.
static bool refusedAsNotBuilt(const std::string &name)
{
  if (!(name == "CPACK" || name == "SC2" || name == "PATTERN" || name == "VIEWER")) return false;
  std::cout << "Algorithm " << name << " is not part of this build: VPC, BDI, FPC and BPC are (see DESIGN.md, \"Out of scope\")." << std::endl;
  return true;
}

// compressor by name (reference main.cpp:85-127); nullptr for a name this build does not evaluate
static comp::DeviceCompressor *makeEvaluator(const std::string &name, const std::string &configPath, unsigned lineSize)
{
  if (name == "VPC") return new comp::VPC(configPath);
  if (name == "BDI") return new comp::BDI(lineSize);
  if (name == "FPC") return new comp::FPC(lineSize);
  if (name == "BPC") return new comp::BPC(lineSize);
  return nullptr;
}

// loader by extension (reference main.cpp:74-83)
static trace::Loader *openTrace(const std::string &tracePath, trace::MemReq_t **memReq)
{
  trace::Loader *loader = trace::OpenByExtension(tracePath, REQ_SIZE, memReq);
  if (!loader) {
    std::cerr << "Unsupported extension." << std::endl;
    abort();
  }
  return loader;
}

// --sector against the trace: a sector is at most a line, and --by counts up to 8 sectors a line
static void requireSector(const Args &a, unsigned traceLineSize)
{
  if ((a.size_histogram || a.has_by) && a.sector > traceLineSize) {
    printf("--sector %u: a sector cannot be larger than the trace's %u-byte lines.\n", a.sector, traceLineSize);
    exit(1);
  }
  if (a.has_by && (traceLineSize + a.sector - 1) / a.sector > comp::ClassReport::Row - 2) {
    printf("--by with --sector %u: the trace's %u-byte lines have more than %zu sectors.\n", a.sector, traceLineSize, comp::ClassReport::Row - 2);
    exit(1);
  }
}

// --pack against the trace: a sector is at most a block, a block at most 1024 sectors
static void requirePack(const Args &a, unsigned traceLineSize)
{
  if (!a.has_pack) return;
  const unsigned long long blockBytes = a.pack * traceLineSize;
  if (a.sector > blockBytes) {
    printf("--pack %llu with --sector %u: a sector cannot be larger than a block of %llu bytes.\n", a.pack, a.sector, blockBytes);
    exit(1);
  }
  if ((blockBytes + a.sector - 1) / a.sector > comp::PackReport::MaxSectors) {
    printf("--pack %llu with --sector %u: a block of %llu bytes has more than %zu sectors.\n", a.pack, a.sector, blockBytes, comp::PackReport::MaxSectors);
    exit(1);
  }
}

// --image against the trace: a sector is at most a block, a block at most 1024 sectors
static void requireImage(const Args &a, unsigned traceLineSize)
{
  if (!a.has_image) return;
  const unsigned long long blockBytes = a.image * traceLineSize;
  if (a.sector > blockBytes) {
    printf("--image %llu with --sector %u: a sector cannot be larger than a block of %llu bytes.\n", a.image, a.sector, blockBytes);
    exit(1);
  }
  if ((blockBytes + a.sector - 1) / a.sector > comp::ImageReport::MaxSectors) {
    printf("--image %llu with --sector %u: a block of %llu bytes has more than %zu sectors.\n", a.image, a.sector, blockBytes, comp::ImageReport::MaxSectors);
    exit(1);
  }
}

// --rewrites against the trace: a granule is at most a line, a line at most 32 granules
static void requireRewrites(const Args &a, unsigned traceLineSize)
{
  if (!a.has_rewrites) return;
  std::string why;
  if (comp::DeviceCompressor::CheckRewriteValues(traceLineSize, (unsigned)a.rewrites, a.rewrite_capacity, why)) return;
  printf("--rewrites %llu over a trace of %u-byte lines: %s.\n", a.rewrites, traceLineSize, why.c_str());
  exit(1);
}

static void writeRewrites(comp::RewriteReport report, const std::string &workloadName, const std::string &outputDirPath, const std::string &saveFileName)
{
  report.Print(workloadName, outputDirPath + "/" + saveFileName + "_results_rewrites.csv");
}

// --snapshot against the trace: a line is 1, 2, 4 or 8 of the trace's requests and at most 256 bytes
static void requireSnapshot(const Args &a, unsigned traceLineSize)
{
  if (!a.has_snapshot) return;
  std::string why;
  if (comp::Snapshot::CheckValues(traceLineSize, a.snapshot_capacity, (unsigned)a.snapshot, why)) return;
  printf("--snapshot %llu over a trace of %u-byte requests: %s.\n", a.snapshot, traceLineSize, why.c_str());
  exit(1);
}

// the snapshot of the trace, evaluated by the evaluator or the set at --snapshot's line size; its own file
template <class Sink>
static comp::SnapshotReport compressSnapshot(Sink &sink, const std::string &tracePath, unsigned unitBytes, const Args &a)
{
  const bool zeroFill = a.snapshot_partial == "zero";
  comp::Snapshot snapshot(unitBytes, a.snapshot_capacity);
  snapshot.AddFile(tracePath);
  snapshot.Evaluate(sink, (unsigned)a.snapshot, zeroFill);
  return snapshot.GetReport((unsigned)a.snapshot, zeroFill);
}

static void writeSnapshot(comp::SnapshotReport report, const std::string &workloadName, const std::string &outputDirPath, const std::string &saveFileName)
{
  report.Print(workloadName, outputDirPath + "/" + saveFileName + "_results_snapshot.csv");
}

static void writeImage(comp::ImageReport report, const std::string &workloadName, const std::string &outputDirPath, const std::string &saveFileName)
{
  report.Print(workloadName, outputDirPath + "/" + saveFileName + "_results_image.csv");
}

static void writePack(comp::PackReport report, const std::string &workloadName, const std::string &outputDirPath, const std::string &saveFileName)
{
  report.Print(workloadName, outputDirPath + "/" + saveFileName + "_results_pack.csv");
}

// --by kernel|rw|mftype: the field of a .log record (MPC_CLASS_LOG_*); 0 for cluster
static int logFieldOf(const std::string &by) { return by == "kernel" ? 1 : by == "rw" ? 2 : by == "mftype" ? 3 : 0; }

static void writeClasses(comp::ClassReport report, const std::string &workloadName, const std::string &outputDirPath,
                         const std::string &saveFileName)
{
  report.Print(workloadName, outputDirPath + "/" + saveFileName + "_results_classes.csv");
}

static void writeSizes(comp::SizeReport report, const std::string &workloadName, const std::string &outputDirPath,
                       const std::string &saveFileName)
{
  report.Print(workloadName, outputDirPath + "/" + saveFileName + "_results_sizes.csv");
}

static void requireLineSize(unsigned traceLineSize, unsigned evaluatorLineSize, bool snapshot = false)
{
  if (evaluatorLineSize == traceLineSize) return;
  if (snapshot) {
    printf("--snapshot %u writes %u-byte lines but the evaluator is configured for %u-byte lines.\n", traceLineSize, traceLineSize, evaluatorLineSize);
    exit(1);
  }
  printf("The trace has %u-byte lines but the evaluator is configured for %u-byte lines.\n", traceLineSize, evaluatorLineSize);
  exit(1);
}

// workload name = <parent directory>_<file stem> (reference main.cpp:141-157); false, with a message, without a '/'
static bool workloadNameOf(const std::string &tracePath, std::string &workloadName)
{
  std::vector<std::string> parts = mpctext::split(tracePath, "/");
  if (parts.size() < 2) {
    std::cout << "The trace path needs at least one '/' (workload name = <directory>_<file>)." << std::endl;
    return false;
  }
  std::string appName = parts[parts.size() - 1];
  mpctext::replace_all(appName, ".log", "");
  mpctext::replace_all(appName, ".npy", "");
  mpctext::replace_all(appName, ".txt", "");
  workloadName = parts[parts.size() - 2] + "_" + appName;
  return true;
}

// The whole trace to a comp::Compressor or a comp::CompressorSet: streamed by the library when the loader allows it,
// else in batches of 64 MiB.
template <class Sink>
static void compressBatches(Sink *sink, trace::Loader *loader)
{
  const std::string path = loader->GetStreamablePath();
  if (!path.empty()) {
    sink->CompressFile(path);
    return;
  }
  const unsigned L = loader->GetCachelineSize();
  const unsigned long long cap = (64ull << 20) / L;
  std::vector<uint8_t> buf((size_t)(cap * L));
  for (;;) {
    unsigned long long n = loader->GetBatch(buf.data(), cap);
    if (n == 0) break;
    sink->CompressBatch(buf.data(), n);
  }
}

// result files (reference main.cpp:129-136)
static void writeResults(comp::CompResult *compStat, const std::string &workloadName, const std::string &outputDirPath,
                         const std::string &saveFileName)
{
  compStat->Print(workloadName, outputDirPath + "/" + saveFileName + "_results.csv");
  compStat->PrintDetail(workloadName, outputDirPath + "/" + saveFileName + "_results_detail.csv");
}

int main(int argc, char **argv)
{
  Args a;
  for (int i = 1; i < argc; i++) {
    const std::string arg = argv[i];
    if (arg == "-h" || arg == "--help") { a.help = true; continue; }
    if (arg == "--per-line") { a.per_line = true; continue; }
    if (arg == "--line-buffer") {
      if (i + 1 >= argc) {
        std::cout << "Option 'line-buffer' is missing an argument" << std::endl;
        exit(1);
      }
      a.per_line = true;
      a.line_buffer = strtoull(argv[++i], nullptr, 10);
      continue;
    }
    if (arg == "--size-histogram") { a.size_histogram = true; continue; }
    if (arg == "--sector" || arg.compare(0, 9, "--sector=") == 0) {
      if (arg == "--sector" && i + 1 >= argc) {
        std::cout << "Option 'sector' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--sector" ? argv[++i] : arg.substr(9);
      char *end = nullptr;
      const unsigned long long bytes = strtoull(value.c_str(), &end, 10);
      if (value.empty() || value[0] < '0' || value[0] > '9' || *end != 0 || bytes == 0 || bytes > 0xffffffffull) {
        std::cout << "--sector takes a number of bytes from 1 to the trace's line size, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.sector = (unsigned)bytes;
      a.has_sector = true;
      continue;
    }
    if (arg == "--pack" || arg.compare(0, 7, "--pack=") == 0) {
      if (arg == "--pack" && i + 1 >= argc) {
        std::cout << "Option 'pack' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--pack" ? argv[++i] : arg.substr(7);
      if (!takeNumber(value, 1ull << 19, a.pack) || a.pack == 0) {
        std::cout << "--pack takes a number of lines from 1 to 524288, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.has_pack = true;
      continue;
    }
    if (arg == "--pack-header" || arg.compare(0, 14, "--pack-header=") == 0) {
      if (arg == "--pack-header" && i + 1 >= argc) {
        std::cout << "Option 'pack-header' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--pack-header" ? argv[++i] : arg.substr(14);
      unsigned long long bits = 0;
      if (!takeNumber(value, 65535, bits)) {
        std::cout << "--pack-header takes a number of bits from 0 to 65535, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.pack_header = (unsigned)bits;
      a.has_pack_header = true;
      continue;
    }
    if (arg == "--image" || arg.compare(0, 8, "--image=") == 0) {
      if (arg == "--image" && i + 1 >= argc) {
        std::cout << "Option 'image' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--image" ? argv[++i] : arg.substr(8);
      if (!takeNumber(value, 1ull << 19, a.image) || a.image == 0) {
        std::cout << "--image takes a number of lines from 1 to 524288, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.has_image = true;
      continue;
    }
    if (arg == "--image-header" || arg.compare(0, 15, "--image-header=") == 0) {
      if (arg == "--image-header" && i + 1 >= argc) {
        std::cout << "Option 'image-header' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--image-header" ? argv[++i] : arg.substr(15);
      unsigned long long bits = 0;
      if (!takeNumber(value, 65535, bits)) {
        std::cout << "--image-header takes a number of bits from 0 to 65535, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.image_header = (unsigned)bits;
      a.has_image_header = true;
      continue;
    }
    if (arg == "--image-capacity" || arg.compare(0, 17, "--image-capacity=") == 0) {
      if (arg == "--image-capacity" && i + 1 >= argc) {
        std::cout << "Option 'image-capacity' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--image-capacity" ? argv[++i] : arg.substr(17);
      if (!takeNumber(value, 1ull << 28, a.image_capacity) || a.image_capacity == 0) {
        std::cout << "--image-capacity takes a number of lines from 1 to 268435456, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.has_image_capacity = true;
      continue;
    }
    if (arg == "--rewrites" || arg.compare(0, 11, "--rewrites=") == 0) {
      if (arg == "--rewrites" && i + 1 >= argc) {
        std::cout << "Option 'rewrites' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--rewrites" ? argv[++i] : arg.substr(11);
      if (!takeNumber(value, 65536, a.rewrites) || a.rewrites == 0) {
        std::cout << "--rewrites takes a granule size in bytes from 1 to the line size, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.has_rewrites = true;
      continue;
    }
    if (arg == "--rewrite-capacity" || arg.compare(0, 19, "--rewrite-capacity=") == 0) {
      if (arg == "--rewrite-capacity" && i + 1 >= argc) {
        std::cout << "Option 'rewrite-capacity' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--rewrite-capacity" ? argv[++i] : arg.substr(19);
      if (!takeNumber(value, 1ull << 28, a.rewrite_capacity) || a.rewrite_capacity == 0) {
        std::cout << "--rewrite-capacity takes a number of lines from 1 to 268435456, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.has_rewrite_capacity = true;
      continue;
    }
    if (arg == "--snapshot" || arg.compare(0, 11, "--snapshot=") == 0) {
      if (arg == "--snapshot" && i + 1 >= argc) {
        std::cout << "Option 'snapshot' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--snapshot" ? argv[++i] : arg.substr(11);
      if (!takeNumber(value, 256, a.snapshot) || a.snapshot == 0) {
        std::cout << "--snapshot takes a line size in bytes, 1, 2, 4 or 8 of the trace's requests and at most 256, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.has_snapshot = true;
      continue;
    }
    if (arg == "--snapshot-partial" || arg.compare(0, 19, "--snapshot-partial=") == 0) {
      if (arg == "--snapshot-partial" && i + 1 >= argc) {
        std::cout << "Option 'snapshot-partial' is missing an argument" << std::endl;
        exit(1);
      }
      a.snapshot_partial = arg == "--snapshot-partial" ? argv[++i] : arg.substr(19);
      if (a.snapshot_partial != "skip" && a.snapshot_partial != "zero") {
        std::cout << "--snapshot-partial takes skip or zero, not \"" << a.snapshot_partial << "\"." << std::endl;
        return 1;
      }
      a.has_snapshot_partial = true;
      continue;
    }
    if (arg == "--snapshot-capacity" || arg.compare(0, 20, "--snapshot-capacity=") == 0) {
      if (arg == "--snapshot-capacity" && i + 1 >= argc) {
        std::cout << "Option 'snapshot-capacity' is missing an argument" << std::endl;
        exit(1);
      }
      const std::string value = arg == "--snapshot-capacity" ? argv[++i] : arg.substr(20);
      if (!takeNumber(value, 1ull << 28, a.snapshot_capacity) || a.snapshot_capacity == 0) {
        std::cout << "--snapshot-capacity takes a number of requests from 1 to 268435456, not \"" << value << "\"." << std::endl;
        return 1;
      }
      a.has_snapshot_capacity = true;
      continue;
    }
    if (arg == "--by" || arg.compare(0, 5, "--by=") == 0) {
      if (arg == "--by" && i + 1 >= argc) {
        std::cout << "Option 'by' is missing an argument" << std::endl;
        exit(1);
      }
      a.by = arg == "--by" ? argv[++i] : arg.substr(5);
      a.has_by = true;
      continue;
    }
    if (take_value(argc, argv, i, arg, "-a", "algorithm", a.algorithm, a.has_algorithm)) continue;
    if (take_value(argc, argv, i, arg, "-i", "input", a.input, a.has_input)) continue;
    if (take_value(argc, argv, i, arg, "-c", "config", a.config, a.has_config)) continue;
    if (take_value(argc, argv, i, arg, "-o", "output", a.output, a.has_output)) continue;
    std::cout << "Option '" << arg << "' does not exist" << std::endl;
    return 1;
  }
  if (a.has_sector && !a.has_pack && !a.has_image) a.size_histogram = true;      // (--sector implies --size-histogram, but not next to --pack or --image)
  std::string algorithm = a.has_algorithm ? a.algorithm : "VPC";
  bool help = a.help;
  if (!a.has_input) help = true;
  // a list of algorithms: checked before anything is opened or written
  std::vector<std::string> list;
  if (algorithm.find(',') != std::string::npos) list = mpctext::split(algorithm, ",");      // ("BDI," has an empty element)
  for (size_t i = 0; i < list.size() && !help; i++) {
    const std::string &n = list[i];
    if (refusedAsNotBuilt(n)) return 1;
    if (!(n == "VPC" || n == "BDI" || n == "FPC" || n == "BPC")) {
      std::cout << "Invalid name of algorithm in the list \"" << algorithm << "\": \"" << n << "\"." << std::endl;
      return 1;
    }
    for (size_t j = 0; j < i; j++)
      if (list[j] == n) {
        std::cout << "Algorithm " << n << " is named twice in the list \"" << algorithm << "\"." << std::endl;
        return 1;
      }
    if (a.per_line) {
      std::cout << "--per-line / --line-buffer evaluate one algorithm: a list of algorithms is fed in batches." << std::endl;
      return 1;
    }
    if (n == "VPC" && !a.has_config) help = true;
  }
  if (algorithm == "VPC" && !a.has_config) help = true;
  if (help) {
    std::cout << kHelp << std::endl;
    return 0;
  }
  // --by: checked before anything is opened or written, one message each
  if (a.has_by) {
    if (!(a.by == "kernel" || a.by == "rw" || a.by == "mftype" || a.by == "cluster")) {
      std::cout << "--by takes one of kernel, rw, mftype and cluster, not \"" << a.by << "\"." << std::endl;
      return 1;
    }
    if (a.by != "cluster" && !trace::IsGpgpuSimLog(a.input)) {
      std::cout << "--by " << a.by << " takes the class from the records of a GPGPU-Sim .log trace: \"" << a.input << "\" is not one." << std::endl;
      return 1;
    }
    bool vpcInList = false;
    for (const std::string &n : list) vpcInList = vpcInList || n == "VPC";
    if (a.by == "cluster" && !vpcInList) {
      std::cout << "--by cluster needs a list of algorithms with a VPC member (-a VPC,BDI,...): its cluster is the class." << std::endl;
      return 1;
    }
    if (a.per_line) {
      std::cout << "--by is evaluated in batches: it does not go with --per-line / --line-buffer." << std::endl;
      return 1;
    }
  }
  // --pack: checked before anything is opened or written, one message each
  if (a.has_pack_header && !a.has_pack) {
    std::cout << "--pack-header adds bits to the blocks of --pack: give --pack N too." << std::endl;
    return 1;
  }
  if (a.has_pack && a.per_line) {
    std::cout << "--pack is evaluated in batches: it does not go with --per-line / --line-buffer." << std::endl;
    return 1;
  }
  // --image: checked before anything is opened or written, one message each
  if ((a.has_image_header || a.has_image_capacity) && !a.has_image) {
    std::cout << "--image-header and --image-capacity belong to --image: give --image N too." << std::endl;
    return 1;
  }
  if (a.has_image && !trace::IsGpgpuSimLog(a.input)) {
    std::cout << "--image takes the line addresses from the records of a GPGPU-Sim .log trace: \"" << a.input << "\" is not one." << std::endl;
    return 1;
  }
  if (a.has_image && a.per_line) {
    std::cout << "--image is evaluated in batches: it does not go with --per-line / --line-buffer." << std::endl;
    return 1;
  }
  // --rewrites: checked before anything is opened or written, one message each
  if (a.has_rewrite_capacity && !a.has_rewrites) {
    std::cout << "--rewrite-capacity belongs to --rewrites: give --rewrites GRANULE too." << std::endl;
    return 1;
  }
  if (a.has_rewrites && !trace::IsGpgpuSimLog(a.input)) {
    std::cout << "--rewrites takes the line addresses from the records of a GPGPU-Sim .log trace: \"" << a.input << "\" is not one." << std::endl;
    return 1;
  }
  if (a.has_rewrites && a.has_snapshot) {
    std::cout << "--rewrites does not go with --snapshot: every address occurs once in a snapshot, nothing is written again." << std::endl;
    return 1;
  }
  if (a.has_rewrites && a.per_line) {
    std::cout << "--rewrites is evaluated in batches: it does not go with --per-line / --line-buffer." << std::endl;
    return 1;
  }
  // --snapshot: checked before anything is opened or written, one message each
  if ((a.has_snapshot_partial || a.has_snapshot_capacity) && !a.has_snapshot) {
    std::cout << "--snapshot-partial and --snapshot-capacity belong to --snapshot: give --snapshot L too." << std::endl;
    return 1;
  }
  if (a.has_snapshot && !trace::IsGpgpuSimLog(a.input)) {
    std::cout << "--snapshot takes the addresses from the records of a GPGPU-Sim .log trace: \"" << a.input << "\" is not one." << std::endl;
    return 1;
  }
  if (a.has_snapshot && a.has_by && a.by != "cluster") {
    std::cout << "--by " << a.by << " does not go with --snapshot: a line assembled from several records has no single record to take the class from." << std::endl;
    return 1;
  }
  if (a.has_snapshot && a.per_line) {
    std::cout << "--snapshot is evaluated in batches: it does not go with --per-line / --line-buffer." << std::endl;
    return 1;
  }
  const std::string tracePath = a.input, configPath = a.config, outputDirPath = a.has_output ? a.output : "";
  if (!list.empty()) return runList(list, tracePath, configPath, outputDirPath, a);

  trace::MemReq_t *memReq = nullptr;
  trace::Loader *loader = openTrace(tracePath, &memReq);
  requireSnapshot(a, loader->GetCachelineSize());
  // the lines that are evaluated: the trace's requests, or with --snapshot the lines assembled from them
  const unsigned lineSize = a.has_snapshot ? (unsigned)a.snapshot : loader->GetCachelineSize();
  requireSector(a, lineSize);
  requirePack(a, lineSize);
  requireImage(a, lineSize);
  requireRewrites(a, lineSize);

  comp::DeviceCompressor *compressor = makeEvaluator(algorithm, configPath, lineSize);
  if (!compressor) {
    if (refusedAsNotBuilt(algorithm)) return 1;
    std::cerr << "Invalid name of algorithm." << std::endl;
    abort();
  }
  const std::string saveFileName = (algorithm == "VPC") ? parseConfig(configPath) : algorithm;

  // The reference's per-line loop (main.cpp:208-248) as a batch loop, unless --per-line / --line-buffer ask for that
  // loop itself or the loader hands out single lines only.
  if (a.line_buffer) compressor->SetLineBuffering(a.line_buffer);
  requireLineSize(lineSize, compressor->GetLineSize(), a.has_snapshot);
  if (a.size_histogram) compressor->EnableSizeHistogram();
  if (a.has_by) {
    compressor->EnableClassStats(a.sector);
    compressor->SetLogClassField(logFieldOf(a.by));
  }
  if (a.has_pack) compressor->EnablePackStats(a.pack, a.sector, a.pack_header);
  if (a.has_image) compressor->EnableImageStats(a.image, a.sector, a.image_header, a.image_capacity);
  if (a.has_rewrites) compressor->EnableRewriteStats((unsigned)a.rewrites, a.rewrite_capacity);
  comp::SnapshotReport snapshotReport(lineSize, false);
  if (a.has_snapshot)
    snapshotReport = compressSnapshot(*compressor, tracePath, loader->GetCachelineSize(), a);
  else if (!a.per_line && (loader->SupportsBatch() || !loader->GetStreamablePath().empty()))
    compressBatches(compressor, loader);
  else
    trace::CompressPerLine(compressor, loader, memReq);
  comp::CompResult *compStat = compressor->GetResult();

  std::string workloadName;
  if (!workloadNameOf(tracePath, workloadName)) return 1;
  if (a.has_snapshot) workloadName += "@snapshot" + std::to_string(a.snapshot);
  std::cout << "comp.ratio: " << mpctext::num(compStat->CompRatio) << std::endl;
  writeResults(compStat, workloadName, outputDirPath, saveFileName);
  if (a.size_histogram) writeSizes(compressor->GetSizeHistogram(a.sector), workloadName, outputDirPath, saveFileName);
  if (a.has_by) writeClasses(compressor->GetClassStats(), workloadName, outputDirPath, saveFileName);
  if (a.has_pack) writePack(compressor->GetPackStats(), workloadName, outputDirPath, saveFileName);
  if (a.has_image) writeImage(compressor->GetImageStats(), workloadName, outputDirPath, saveFileName);
  if (a.has_rewrites) writeRewrites(compressor->GetRewriteStats(), workloadName, outputDirPath, saveFileName);
  if (a.has_snapshot) writeSnapshot(snapshotReport, workloadName, outputDirPath, saveFileName);

  delete memReq;      // (the reference leaks its request object)
  delete loader;
  delete compressor;
  return 0;
}

// -a with a list: one pass over the trace for all of them, then each algorithm's own result files and one
// "<name> comp.ratio: <ratio>" line each, in list order.  With --size-histogram: each algorithm's sizes file, then the
// per-line best of the list, "BEST comp.ratio: <original bits / (best bits + lines x tag bits)>" and BEST_results_sizes.csv.
static int runList(const std::vector<std::string> &names, const std::string &tracePath, const std::string &configPath,
                   const std::string &outputDirPath, const Args &a)
{
  std::string workloadName;
  if (!workloadNameOf(tracePath, workloadName)) return 1;
  if (a.has_snapshot) workloadName += "@snapshot" + std::to_string(a.snapshot);

  trace::MemReq_t *memReq = nullptr;
  trace::Loader *loader = openTrace(tracePath, &memReq);
  requireSnapshot(a, loader->GetCachelineSize());
  const unsigned lineSize = a.has_snapshot ? (unsigned)a.snapshot : loader->GetCachelineSize();
  requireSector(a, lineSize);
  requirePack(a, lineSize);
  requireImage(a, lineSize);
  requireRewrites(a, lineSize);
  std::vector<comp::DeviceCompressor *> evaluators;
  std::vector<comp::Compressor *> members;
  for (const std::string &n : names) {
    evaluators.push_back(makeEvaluator(n, configPath, lineSize));      // (main() has checked the names)
    members.push_back(evaluators.back());
    requireLineSize(lineSize, members.back()->GetLineSize(), a.has_snapshot);
    if (a.size_histogram) evaluators.back()->EnableSizeHistogram();
  }
  {
    comp::CompressorSet set(members);
    if (a.size_histogram) set.EnableBest();
    if (a.has_by) {
      set.EnableClassStats(a.sector);
      if (a.by == "cluster") {
        size_t vpc = 0;
        while (names[vpc] != "VPC") vpc++;      // (main() has checked that there is one)
        set.ClassFromMember(vpc);
      } else {
        set.SetLogClassField(logFieldOf(a.by));
      }
    }
    if (a.has_pack) set.EnablePackStats(a.pack, a.sector, a.pack_header);      // (behind EnableBest: the best of the list gets its table)
    if (a.has_image) set.EnableImageStats(a.image, a.sector, a.image_header, a.image_capacity);
    if (a.has_rewrites) set.EnableRewriteStats((unsigned)a.rewrites, a.rewrite_capacity);
    comp::SnapshotReport snapshotReport(lineSize, false);
    if (a.has_snapshot)
      snapshotReport = compressSnapshot(set, tracePath, loader->GetCachelineSize(), a);
    else
      compressBatches(&set, loader);
    for (size_t i = 0; i < names.size(); i++) {
      comp::CompResult *compStat = set.GetResult(i);
      const std::string saveFileName = (names[i] == "VPC") ? parseConfig(configPath) : names[i];
      std::cout << names[i] << " comp.ratio: " << mpctext::num(compStat->CompRatio) << std::endl;
      writeResults(compStat, workloadName, outputDirPath, saveFileName);
      if (a.size_histogram) writeSizes(evaluators[i]->GetSizeHistogram(a.sector), workloadName, outputDirPath, saveFileName);
      if (a.has_by) writeClasses(set.GetClassStats(i), workloadName, outputDirPath, saveFileName);
      if (a.has_pack) writePack(set.GetPackStats(i), workloadName, outputDirPath, saveFileName);
      if (a.has_image) writeImage(set.GetImageStats(i), workloadName, outputDirPath, saveFileName);
      if (a.has_rewrites) writeRewrites(set.GetRewriteStats(i), workloadName, outputDirPath, saveFileName);
      if (a.has_snapshot) writeSnapshot(snapshotReport, workloadName, outputDirPath, saveFileName);
    }
    if (a.size_histogram) {
      const comp::BestReport best = set.GetBest(a.sector);
      std::cout << "BEST comp.ratio: " << mpctext::num(best.CompRatio()) << std::endl;
      writeSizes(best.Sizes, workloadName, outputDirPath, "BEST");
      if (a.has_by) writeClasses(set.GetClassStats(comp::CompressorSet::BestMember), workloadName, outputDirPath, "BEST");
      if (a.has_pack) writePack(set.GetPackStats(comp::CompressorSet::BestMember), workloadName, outputDirPath, "BEST");
    }
  }
  delete memReq;
  delete loader;
  for (comp::Compressor *c : members) delete c;
  return 0;
}
