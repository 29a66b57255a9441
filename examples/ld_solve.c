/* Plain-C consumer of libelf_amd.so: a life-and-death problem solved exactly -- the straight three in the corner.
 *   gcc -std=c11 -O2 -I include examples/ld_solve.c -o ld_solve -L elf_amd/lib -lelf_amd -Wl,-rpath,$PWD/elf_amd/lib
 *   ./ld_solve [b|w] [depth] [zobrist21.bin]
 * Black's eye space is (0,0) (1,0) (2,0): the side to move (default b) lives or kills at (1,0), the middle.  Prints the frame of
 * the problem, then per first move its minimax value (alive / unsettled / dead for Black's group) and the nodes searched. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "elf_amd.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d (%s)\n", #x, rc_, elfgo_error_string(rc_)); return 1; } } while (0)
#define N 9
#define NA (N * N + 1)

/* row = y, column = x, X Black, O White */
static const char* ROWS[3] = {"...XO....", "XXXXO....", "OOOOO...."};
static const char* WORD[3] = {"dead", "unsettled", "alive"};

int main(int argc, char** argv) {
  const uint8_t mover = (argc > 1 && argv[1][0] == 'w') ? 2 : 1;
  const int depth = argc > 2 ? atoi(argv[2]) : 5;
  const char* zpath = argc > 3 ? argv[3] : "elf_amd/data/zobrist21.bin";
  uint64_t zob[441];
  FILE* f = fopen(zpath, "rb");
  if (!f || fread(zob, sizeof(uint64_t), 441, f) != 441) { fprintf(stderr, "cannot read %s\n", zpath); return 1; }
  fclose(f);
  if (depth < 0 || depth > elfgo_ld_solve_max_depth()) { fprintf(stderr, "depth must be 0 .. %d\n", elfgo_ld_solve_max_depth()); return 1; }
  uint8_t stones[N * N];
  memset(stones, 0, sizeof(stones));
  for (int y = 0; y < 3; ++y)
    for (int x = 0; x < N; ++x) stones[x * N + y] = ROWS[y][x] == 'X' ? 1 : ROWS[y][x] == 'O' ? 2 : 0;   /* a = x*N + y */
  const int32_t box[4] = {0, 0, 5, 3};   /* left, top, right, bottom: half-open */
  ElfGoEngine* e = NULL;
  CHECK(elfgo_create(N, 1, 0, zob, &e));      /* the first (N+2)^2 constants serve the 9x9 board */
  void *d_stones = NULL, *d_mover = NULL, *d_ok = NULL, *d_box = NULL, *d_info = NULL, *d_value = NULL, *d_nodes = NULL;
  CHECK(elfgo_malloc(&d_stones, sizeof(stones)));
  CHECK(elfgo_malloc(&d_mover, 1));
  CHECK(elfgo_malloc(&d_ok, 1));
  CHECK(elfgo_malloc(&d_box, sizeof(box)));
  CHECK(elfgo_malloc(&d_info, 8 * sizeof(int32_t)));
  CHECK(elfgo_malloc(&d_value, NA));
  CHECK(elfgo_malloc(&d_nodes, NA * sizeof(int32_t)));
  CHECK(elfgo_memcpy_h2d(d_stones, stones, sizeof(stones)));
  CHECK(elfgo_memcpy_h2d(d_mover, &mover, 1));
  CHECK(elfgo_memcpy_h2d(d_box, box, sizeof(box)));
  CHECK(elfgo_reset(e, NULL, 1, NULL));
  CHECK(elfgo_setup(e, NULL, (const uint8_t*)d_stones, (const uint8_t*)d_mover, 1, (uint8_t*)d_ok, NULL));
  /* threshold 3: throw-ins of one or two stones stay in the move list; attackers NULL: GuessLDAttacker names the attacker */
  CHECK(elfgo_ld_solve(e, NULL, 1, (const int32_t*)d_box, NULL, depth, 1 << 16, 3, (int32_t*)d_info, (int8_t*)d_value, (int32_t*)d_nodes, NULL));
  CHECK(elfgo_sync(e, NULL));
  uint8_t ok = 0;
  int32_t info[8], nodes[NA];
  int8_t value[NA];
  CHECK(elfgo_memcpy_d2h(&ok, d_ok, 1));
  CHECK(elfgo_memcpy_d2h(info, d_info, sizeof(info)));
  CHECK(elfgo_memcpy_d2h(value, d_value, sizeof(value)));
  CHECK(elfgo_memcpy_d2h(nodes, d_nodes, sizeof(nodes)));
  if (!ok) { fprintf(stderr, "the position was refused\n"); return 1; }
  printf("box %d %d %d %d attacker %c defender %c to move %c now %s depth %d\n", info[0], info[1], info[2], info[3], " bw"[info[4]],
         " bw"[info[5]], " bw"[info[6]], WORD[info[7]], depth);
  for (int a = 0; a < NA; ++a) {
    if (value[a] == -1) continue;
    if (a == N * N) printf("pass ");
    else printf("(%d,%d)", a / N, a % N);
    printf(" %s nodes %d\n", value[a] < 0 ? "cut" : WORD[value[a]], nodes[a]);
  }
  CHECK(elfgo_free(d_stones));
  CHECK(elfgo_free(d_mover));
  CHECK(elfgo_free(d_ok));
  CHECK(elfgo_free(d_box));
  CHECK(elfgo_free(d_info));
  CHECK(elfgo_free(d_value));
  CHECK(elfgo_free(d_nodes));
  CHECK(elfgo_destroy(e));
  return 0;
}
