/* Plain-C consumer of libelf_amd.so: Monte-Carlo ownership of a 9x9 position after `plies` plies of random play.
 *   gcc -std=c11 -O2 -I include examples/ownership.c -o ownership -L elf_amd/lib -lelf_amd -Wl,-rpath,$PWD/elf_amd/lib
 *   ./ownership [plies] [playouts] [zobrist21.bin]
 * Prints (black - white) / playouts per point in board orientation (top row first) and the mean score. */
#include <stdio.h>
#include <stdlib.h>

#include "elf_amd.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d (%s)\n", #x, rc_, elfgo_error_string(rc_)); return 1; } } while (0)
#define N 9

int main(int argc, char** argv) {
  const int plies = argc > 1 ? atoi(argv[1]) : 40, playouts = argc > 2 ? atoi(argv[2]) : 1024;
  const char* zpath = argc > 3 ? argv[3] : "elf_amd/data/zobrist21.bin";
  uint64_t zob[441];
  FILE* f = fopen(zpath, "rb");
  if (!f || fread(zob, sizeof(uint64_t), 441, f) != 441) { fprintf(stderr, "cannot read %s\n", zpath); return 1; }
  fclose(f);
  ElfGoEngine* e = NULL;
  ElfGoOwnership* own = NULL;
  CHECK(elfgo_create(N, 1, 0, zob, &e));      /* the first (N+2)^2 constants serve the 9x9 board */
  CHECK(elfgo_own_create(e, 0, &own));
  const uint64_t seed = 1;
  void *d_seed = NULL, *d_out = NULL, *d_counts = NULL, *d_stats = NULL;
  CHECK(elfgo_malloc(&d_seed, sizeof(seed)));
  CHECK(elfgo_malloc(&d_out, 4 * sizeof(uint32_t)));
  CHECK(elfgo_malloc(&d_counts, 2 * N * N * sizeof(int32_t)));
  CHECK(elfgo_malloc(&d_stats, 4 * sizeof(int64_t)));
  CHECK(elfgo_memcpy_h2d(d_seed, &seed, sizeof(seed)));
  CHECK(elfgo_playout(e, NULL, (const uint64_t*)d_seed, 1, plies, (uint32_t*)d_out, NULL));      /* the position to judge */
  CHECK(elfgo_own_run(own, NULL, (const uint64_t*)d_seed, 1, playouts, 1 << 20, 7.5f, (int32_t*)d_counts, (int64_t*)d_stats, NULL));
  CHECK(elfgo_sync(e, NULL));
  int32_t counts[2][N * N];
  int64_t stats[4];
  CHECK(elfgo_memcpy_d2h(counts, d_counts, sizeof(counts)));
  CHECK(elfgo_memcpy_d2h(stats, d_stats, sizeof(stats)));
  for (int y = N - 1; y >= 0; --y) {
    for (int x = 0; x < N; ++x) printf(" %5.2f", (double)(counts[0][x * N + y] - counts[1][x * N + y]) / playouts);
    printf("\n");
  }
  printf("playouts %d mean score %+.2f black wins %lld super-ko endings %lld steps %lld\n", playouts,
         (double)stats[0] / playouts - 7.5, (long long)stats[1], (long long)stats[2], (long long)stats[3]);
  CHECK(elfgo_free(d_seed));
  CHECK(elfgo_free(d_out));
  CHECK(elfgo_free(d_counts));
  CHECK(elfgo_free(d_stats));
  CHECK(elfgo_own_destroy(own));
  CHECK(elfgo_destroy(e));
  return 0;
}
