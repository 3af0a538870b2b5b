// SC2.h -- the SC2 Huffman baseline behind the reference's class name (reference src/compressor/SC2.h);
// evaluation on the MI355X via libmpc_hip.so (mpc_create_sc2): the warm-up counts, the table selection and the
// sizing run on the device, the Huffman heap on the host, as the reference builds it.
#ifndef MPC_HOST_SC2_H
#define MPC_HOST_SC2_H

#include "CompResult.h"
#include "Compressor.h"

#define SC2_ENTRIES 1024
#define WARM_UP_CNT 1000000

namespace comp
{

class SC2 : public Compressor
{
public:
  // warmupCnt: lines whose words only feed the frequency table (each costs lineSize / 4 x 33 bits); the table is built
  // when line warmupCnt arrives.  The reference driver passes max(10000, min(numLines / 100, WARM_UP_CNT)).
  SC2(unsigned lineSize, unsigned warmupCnt = 100000);
  virtual ~SC2();
  virtual unsigned CompressLine(std::vector<uint8_t> &dataLine);
  virtual CompResult *GetResult();
  virtual void CompressBatch(const uint8_t *lines, unsigned long long n);
  virtual unsigned long long CompressFile(const std::string &tracePath);
  virtual unsigned GetLineSize() { return m_LineSize; }
  virtual mpc_handle *DeviceHandle() { FlushLines(); m_Started = true; return m_Handle; }
  // Before the first line only: the evaluator is created again with the new warm-up count.
  void SetSamplingCnt(unsigned cnt);

private:
  mpc_handle *m_Handle;
  unsigned m_LineSize;
  bool m_Started;
};

}  // namespace comp

#endif
