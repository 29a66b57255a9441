// The MCTS translation unit of libelf_amd.so: mcts_capi.hip as it stands, plus the entry points that need its private types
// (struct ElfMcts, tree_of<N>()) but are not part of the profiled search path.  mcts_capi.hip is one of
// elf_amd._lib.KERNEL_SOURCES -- the committed PMC profiles are only priced while its bytes stand -- so additions live in
// headers of their own and GNUmakefile compiles this file in its place.
#include "mcts_capi.hip"

#include "mcts_analyze_host.h"
