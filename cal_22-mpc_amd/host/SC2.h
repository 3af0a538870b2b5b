// SC2.h -- the SC2 Huffman baseline behind the reference's class name (reference src/compressor/SC2.h);
// evaluation on the MI355X via libmpc_hip.so (mpc_create_sc2): the warm-up counts, the table selection and the
// sizing run on the device, the Huffman heap on the host, as the reference builds it.
#ifndef MPC_HOST_SC2_H
#define MPC_HOST_SC2_H

#include "CompResult.h"
#include "DeviceCompressor.h"

#define SC2_ENTRIES 1024
#define WARM_UP_CNT 1000000

namespace comp
{

class SC2 : public DeviceCompressor
{
public:
  // warmupCnt: lines whose words only feed the frequency table (each costs lineSize / 4 x 33 bits); the table is built
  // when line warmupCnt arrives.  The reference driver passes max(10000, min(numLines / 100, WARM_UP_CNT)).
  SC2(unsigned lineSize, unsigned warmupCnt = 100000);
  // Before the first line only: the evaluator is created again with the new warm-up count.
  void SetSamplingCnt(unsigned cnt);

protected:
  // CompResult only (SC2's PrintDetail is empty)
  virtual void LoadResult(const uint64_t *v);
};

}  // namespace comp

#endif
