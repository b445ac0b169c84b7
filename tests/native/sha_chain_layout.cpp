// Prints the layout of the hash queue's chain record (cess_amd/csrc/kernels.h) as the host
// compiler sees it: "sizeof <bytes>" and "<field> <offset> <size>" per field, for
// tests/test_hashq_check_decl.py.
#include <cstddef>
#include <cstdio>

#include "../../cess_amd/csrc/kernels.h"

#define FIELD(f) \
  std::printf(#f " %zu %zu\n", offsetof(cec::ShaChain, f), sizeof(cec::ShaChain::f))

int main() {
  std::printf("sizeof %zu\n", sizeof(cec::ShaChain));
  FIELD(src);
  FIELD(len);
  FIELD(blk);
  FIELD(hex);
  FIELD(h);
  FIELD(pre_hex);
  FIELD(pre_blk);
  FIELD(pre_h);
  FIELD(expect);
  FIELD(ok);
  return 0;
}
