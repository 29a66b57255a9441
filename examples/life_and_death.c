/* Plain-C consumer of libelf_amd.so: a life-and-death problem read by region playouts -- the straight three in the corner.
 *   gcc -std=c11 -O2 -I include examples/life_and_death.c -o life_and_death -L elf_amd/lib -lelf_amd -Wl,-rpath,$PWD/elf_amd/lib
 *   ./life_and_death [b|w] [playouts] [zobrist21.bin]
 * Black's eye space is (0,0) (1,0) (2,0): the side to move (default b) lives or kills at (1,0), the middle.  Prints the frame of
 * the problem, then per first move how many playouts started there, in how many the defender ended with a two-eyed group in the
 * box ("lived") and in how many with any stone in the box ("survived"). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "elf_amd.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d (%s)\n", #x, rc_, elfgo_error_string(rc_)); return 1; } } while (0)
#define N 9
#define NA (N * N + 1)

/* row = y, column = x, X Black, O White */
static const char* ROWS[3] = {"...XO....", "XXXXO....", "OOOOO...."};

int main(int argc, char** argv) {
  const uint8_t mover = (argc > 1 && argv[1][0] == 'w') ? 2 : 1;
  const int playouts = argc > 2 ? atoi(argv[2]) : 256;
  const char* zpath = argc > 3 ? argv[3] : "elf_amd/data/zobrist21.bin";
  uint64_t zob[441];
  FILE* f = fopen(zpath, "rb");
  if (!f || fread(zob, sizeof(uint64_t), 441, f) != 441) { fprintf(stderr, "cannot read %s\n", zpath); return 1; }
  fclose(f);
  uint8_t stones[N * N];
  memset(stones, 0, sizeof(stones));
  for (int y = 0; y < 3; ++y)
    for (int x = 0; x < N; ++x) stones[x * N + y] = ROWS[y][x] == 'X' ? 1 : ROWS[y][x] == 'O' ? 2 : 0;   /* a = x*N + y */
  const int32_t box[4] = {0, 0, 5, 3};   /* left, top, right, bottom: half-open */
  const uint64_t seed = 1;
  ElfGoEngine* e = NULL;
  ElfGoOwnership* own = NULL;
  CHECK(elfgo_create(N, 1, 0, zob, &e));      /* the first (N+2)^2 constants serve the 9x9 board */
  CHECK(elfgo_own_create(e, 0, &own));        /* the playouts' scratch: the ownership handle */
  void *d_stones = NULL, *d_mover = NULL, *d_ok = NULL, *d_box = NULL, *d_seed = NULL, *d_info = NULL, *d_stats = NULL, *d_first = NULL;
  CHECK(elfgo_malloc(&d_stones, sizeof(stones)));
  CHECK(elfgo_malloc(&d_mover, 1));
  CHECK(elfgo_malloc(&d_ok, 1));
  CHECK(elfgo_malloc(&d_box, sizeof(box)));
  CHECK(elfgo_malloc(&d_seed, sizeof(seed)));
  CHECK(elfgo_malloc(&d_info, 8 * sizeof(int32_t)));
  CHECK(elfgo_malloc(&d_stats, 8 * sizeof(int64_t)));
  CHECK(elfgo_malloc(&d_first, 3 * NA * sizeof(int32_t)));
  CHECK(elfgo_memcpy_h2d(d_stones, stones, sizeof(stones)));
  CHECK(elfgo_memcpy_h2d(d_mover, &mover, 1));
  CHECK(elfgo_memcpy_h2d(d_box, box, sizeof(box)));
  CHECK(elfgo_memcpy_h2d(d_seed, &seed, sizeof(seed)));
  CHECK(elfgo_reset(e, NULL, 1, NULL));
  CHECK(elfgo_setup(e, NULL, (const uint8_t*)d_stones, (const uint8_t*)d_mover, 1, (uint8_t*)d_ok, NULL));
  /* threshold 3: throw-ins of one or two stones stay in the move list; attackers NULL: GuessLDAttacker names the attacker */
  CHECK(elfgo_ld_run(own, NULL, (const uint64_t*)d_seed, 1, playouts, 1 << 20, 3, (const int32_t*)d_box, NULL, (int32_t*)d_info,
                     (int64_t*)d_stats, (int32_t*)d_first, NULL));
  CHECK(elfgo_sync(e, NULL));
  uint8_t ok = 0;
  int32_t info[8], first[3][NA];
  int64_t stats[8];
  CHECK(elfgo_memcpy_d2h(&ok, d_ok, 1));
  CHECK(elfgo_memcpy_d2h(info, d_info, sizeof(info)));
  CHECK(elfgo_memcpy_d2h(stats, d_stats, sizeof(stats)));
  CHECK(elfgo_memcpy_d2h(first, d_first, sizeof(first)));
  if (!ok) { fprintf(stderr, "the position was refused\n"); return 1; }
  printf("box %d %d %d %d attacker %c defender %c to move %c lives now %d\n", info[0], info[1], info[2], info[3], " bw"[info[4]],
         " bw"[info[5]], " bw"[info[6]], info[7]);
  printf("playouts %d lived %lld survived %lld super-ko endings %lld steps %lld\n", playouts, (long long)stats[0], (long long)stats[1],
         (long long)stats[4], (long long)stats[5]);
  for (int a = 0; a < NA; ++a) {
    if (!first[0][a]) continue;
    if (a == N * N) printf("pass ");
    else printf("(%d,%d)", a / N, a % N);
    printf(" playouts %d lived %d survived %d\n", first[0][a], first[1][a], first[2][a]);
  }
  CHECK(elfgo_free(d_stones));
  CHECK(elfgo_free(d_mover));
  CHECK(elfgo_free(d_ok));
  CHECK(elfgo_free(d_box));
  CHECK(elfgo_free(d_seed));
  CHECK(elfgo_free(d_info));
  CHECK(elfgo_free(d_stats));
  CHECK(elfgo_free(d_first));
  CHECK(elfgo_own_destroy(own));
  CHECK(elfgo_destroy(e));
  return 0;
}
