/* Plain-C consumer of libelf_amd.so: Benson's unconditional life of a two-eyed corner group.
 *   gcc -std=c11 -O2 -I include examples/pass_alive.c -o pass_alive -L elf_amd/lib -lelf_amd -Wl,-rpath,$PWD/elf_amd/lib
 *   ./pass_alive [zobrist21.bin]
 * Black's corner group has the eyes (0,0) and (2,0), the second one with a dead White stone beside its empty point; White's wall
 * has no eye.  Prints the top rows of the map -- A / a: a Black / White stone of a pass-alive chain, s / t: a safe point of Black /
 * White -- and the summary; expected:
 *   sAssAO...
 *   AAAAAO...
 *   OOOOOO...
 *   black: chains 1 stones 7 safe points 3 rounds 1
 *   white: chains 0 stones 0 safe points 0 rounds 2 */
#include <stdio.h>
#include <string.h>

#include "elf_amd.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d (%s)\n", #x, rc_, elfgo_error_string(rc_)); return 1; } } while (0)
#define N 9
#define ROWS_SHOWN 3

/* row = y, column = x, X Black, O White */
static const char* ROWS[ROWS_SHOWN] = {".X.OXO...", "XXXXXO...", "OOOOOO..."};

int main(int argc, char** argv) {
  const char* zpath = argc > 1 ? argv[1] : "elf_amd/data/zobrist21.bin";
  uint64_t zob[441];
  FILE* f = fopen(zpath, "rb");
  if (!f || fread(zob, sizeof(uint64_t), 441, f) != 441) { fprintf(stderr, "cannot read %s\n", zpath); return 1; }
  fclose(f);
  uint8_t stones[N * N];
  memset(stones, 0, sizeof(stones));
  for (int y = 0; y < ROWS_SHOWN; ++y)
    for (int x = 0; x < N; ++x) stones[x * N + y] = ROWS[y][x] == 'X' ? 1 : ROWS[y][x] == 'O' ? 2 : 0;   /* a = x*N + y */
  ElfGoEngine* e = NULL;
  CHECK(elfgo_create(N, 1, 0, zob, &e));      /* the first (N+2)^2 constants serve the 9x9 board */
  void *d_stones = NULL, *d_ok = NULL, *d_map = NULL, *d_summary = NULL;
  CHECK(elfgo_malloc(&d_stones, sizeof(stones)));
  CHECK(elfgo_malloc(&d_ok, 1));
  CHECK(elfgo_malloc(&d_map, N * N));
  CHECK(elfgo_malloc(&d_summary, 8 * sizeof(int32_t)));
  CHECK(elfgo_memcpy_h2d(d_stones, stones, sizeof(stones)));
  CHECK(elfgo_reset(e, NULL, 1, NULL));
  CHECK(elfgo_setup(e, NULL, (const uint8_t*)d_stones, NULL, 1, (uint8_t*)d_ok, NULL));
  CHECK(elfgo_pass_alive(e, NULL, 1, (uint8_t*)d_map, (int32_t*)d_summary, NULL));
  CHECK(elfgo_sync(e, NULL));
  uint8_t ok = 0, map[N * N];
  int32_t summary[8];
  CHECK(elfgo_memcpy_d2h(&ok, d_ok, 1));
  CHECK(elfgo_memcpy_d2h(map, d_map, sizeof(map)));
  CHECK(elfgo_memcpy_d2h(summary, d_summary, sizeof(summary)));
  if (!ok) { fprintf(stderr, "the position was refused\n"); return 1; }
  for (int y = 0; y < ROWS_SHOWN; ++y) {
    for (int x = 0; x < N; ++x) {
      const uint8_t m = map[x * N + y];
      putchar((m & 1) ? 'A' : (m & 2) ? 'a' : (m & 4) ? 's' : (m & 8) ? 't' : stones[x * N + y] == 1 ? 'X' : stones[x * N + y] == 2 ? 'O' : '.');
    }
    putchar('\n');
  }
  for (int c = 0; c < 2; ++c)
    printf("%s: chains %d stones %d safe points %d rounds %d%s\n", c ? "white" : "black", summary[4 * c], summary[4 * c + 1],
           summary[4 * c + 2], summary[4 * c + 3] & 0x7FFFFFFF, summary[4 * c + 3] < 0 ? " (bound hit)" : "");
  CHECK(elfgo_free(d_stones));
  CHECK(elfgo_free(d_ok));
  CHECK(elfgo_free(d_map));
  CHECK(elfgo_free(d_summary));
  CHECK(elfgo_destroy(e));
  return 0;
}
