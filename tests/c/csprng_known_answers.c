/* The host layer's generator (csrc/host/csprng.c) driven from a script on standard input, for tests/test_keygen_known_answers.py: built from the host layer's
 * SOURCES (mc_chacha20_block has hidden visibility in the library) into a process of its own, so the stream positions do not depend on what else ran before.
 * No GPU involved: the engine is never started.  One command per line, one line of output per command:
 *   block K0 .. K7 COUNTER NONCE   (hex)       16 output words of mc_chacha20_block
 *   seed S                         (hex)       mosfhet_seed
 *   bytes N [N ...]                            generate_random_bytes for each N, the bytes of all requests in a row (8 guard bytes behind each are checked)
 *   thread N [N ...]                           the same on a thread of its own (joined before the next command)
 *   normal SIGMA COUNT             (hex float) COUNT results of generate_normal_random as hex floats
 *   torus SIGMA COUNT                          generate_torus_normal_random_array of COUNT words
 *   rndseed                                    the words generate_rnd_seed writes (a fifth word behind them is checked) */
#include <inttypes.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mosfhet.h>
#include "host/compat_internal.h"

static void *do_bytes(void *arg) {
  char *p = (char *)arg;
  for (;;) {
    char *end;
    const unsigned long n = strtoul(p, &end, 10);
    if (end == p) break;
    p = end;
    uint8_t *buf = (uint8_t *)malloc(n + 8);
    memset(buf, 0xA5, n + 8);
    generate_random_bytes(n, buf);
    for (int i = 0; i < 8; i++)
      if (buf[n + i] != 0xA5) { printf("OVERRUN"); break; }
    for (unsigned long i = 0; i < n; i++) printf("%02x", buf[i]);
    free(buf);
  }
  printf("\n");
  return NULL;
}

int main(void) {
  static char line[4096];
  while (fgets(line, sizeof(line), stdin)) {
    char *arg = strchr(line, ' ');
    if (arg) *arg++ = 0; else { line[strcspn(line, "\n")] = 0; arg = line + strlen(line); }
    if (!strcmp(line, "block")) {
      uint32_t key[8], out[16];
      for (int i = 0; i < 8; i++) key[i] = (uint32_t)strtoul(arg, &arg, 16);
      const uint64_t counter = strtoull(arg, &arg, 16), nonce = strtoull(arg, &arg, 16);
      mc_chacha20_block(out, key, counter, nonce);
      for (int i = 0; i < 16; i++) printf("%08x%c", out[i], i == 15 ? '\n' : ' ');
    } else if (!strcmp(line, "seed")) {
      mosfhet_seed(strtoull(arg, NULL, 16));
      printf("seeded\n");
    } else if (!strcmp(line, "bytes")) {
      do_bytes(arg);
    } else if (!strcmp(line, "thread")) {
      pthread_t th;
      if (pthread_create(&th, NULL, do_bytes, arg)) return 2;
      pthread_join(th, NULL);
    } else if (!strcmp(line, "normal")) {
      const double sigma = strtod(arg, &arg);
      const long count = strtol(arg, NULL, 10);
      for (long i = 0; i < count; i++) printf("%a%c", generate_normal_random(sigma), i == count - 1 ? '\n' : ' ');
    } else if (!strcmp(line, "torus")) {
      const double sigma = strtod(arg, &arg);
      const long count = strtol(arg, NULL, 10);
      Torus *out = (Torus *)calloc((size_t)count + 1, sizeof(Torus));
      generate_torus_normal_random_array(out, sigma, (int)count);
      if (out[count]) printf("OVERRUN");
      for (long i = 0; i < count; i++) printf("%016" PRIx64 "%c", out[i], i == count - 1 ? '\n' : ' ');
      free(out);
    } else if (!strcmp(line, "rndseed")) {
      uint64_t w[5] = {0, 0, 0, 0, 0x5A5A5A5A5A5A5A5Aull};
      generate_rnd_seed(w);
      if (w[4] != 0x5A5A5A5A5A5A5A5Aull) printf("OVERRUN");
      printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", w[0], w[1], w[2], w[3]);
    } else {
      printf("unknown command %s\n", line);
      return 1;
    }
  }
  return 0;
}
