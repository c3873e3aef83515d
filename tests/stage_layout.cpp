// stage_layout — rtg_stage.h's layout from the command line, for
// tests/test_stage_host.py: each argument is one list of part sizes, "0,16,1";
// its line of output is every part's offset ("-": an absent part) and the total.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rtg_stage.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::vector<size_t> bytes;
    for (char* s = argv[a]; *s;) {
      bytes.push_back((size_t)strtoull(s, &s, 10));
      if (*s == ',') ++s;
    }
    std::vector<size_t> at(bytes.size());
    const size_t total = rtg::stage_layout(bytes.data(), bytes.size(), at.data());
    for (size_t o : at) {
      if (o == rtg::kStageAbsent) printf("- ");
      else printf("%zu ", o);
    }
    printf("%zu\n", total);
  }
  return 0;
}
