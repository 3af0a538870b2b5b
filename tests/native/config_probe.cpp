// config_probe.cpp -- CPU test driver (built with -fsanitize=address,undefined) for the
// JSON reader and the VPC configuration model: parse, validate, plan, read the plan back; never touches HIP.
//   config_probe FILE...   -> one line per file: rc, path, message (read: a sum over the read-back of a fast plan)
#include <cstdio>
#include <string>

#include "mpc_config.h"

int main(int argc, char **argv)
{
  for (int i = 1; i < argc; i++) {
    std::string text, err;
    if (!mpc::read_file(argv[i], text)) { printf("%s: unreadable\n", argv[i]); continue; }
    mpc::VpcConfig cfg;
    int rc = mpc::parse_vpc_config(text, cfg, err);
    if (rc == 0) {
      mpc::VpcPlan plan;
      mpc::build_vpc_plan(cfg, plan);
      long read = 0;
      for (int q = 0; plan.fast && q < cfg.n_pred; q++) {
        mpc::VpcModuleRead rb;
        mpc::read_back_vpc_module(plan, q, rb);
        for (int v : rb.base) read += v;
        for (int v : rb.shift) read += v;
        for (int v : rb.diff) read += v;
        read += (long)std::string(rb.base_form).size();
      }
      printf("%s: rc 0 L %d M %d path %s tab %zu gtab %zu read %ld\n", argv[i], cfg.L, cfg.M, plan.fast ? "fast" : "generic",
             plan.tab.size(), plan.gtab.size(), read);
    } else {
      printf("%s: rc %d %s\n", argv[i], rc, err.c_str());
    }
  }
  return 0;
}
