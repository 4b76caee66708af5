// client_kernels.h -- the client half on the device: encrypting and opening batches of samples under a secret key (include/mosfhet_hip.h: mosfhet_hip_client_key_create,
// mosfhet_hip_tlwe_encrypt_batch .. mosfhet_hip_trlwe_phase_batch; the reference's tlwe_new_sample / tlwe_phase, src/tlwe.c, trlwe_new_sample / trlwe_phase,
// src/trlwe.c:296-331, trgsw_new_monomial_sample, src/trgsw.c:152-168).  Own code.
//   * No kernel of its own: the bodies below are run-time kinds of two generator kernels (keygen_kernels.h: ClientParams) -- client_ring_body (TRLWE / TRGSW rows,
//     TRLWE phases) in trlwe_poly_keygen_kernel, client_lwe_body (TLWE samples, TLWE phases) in tlwe_ksk_keygen_kernel -- launched by capi_client.inc.
//   * The key arrives as an image the host packed at creation (capi_client.inc): the nonzero coefficients of the TRLWE key as words (value << 16) | position, then the
//     LWE key as one int per coefficient.  No kernel scans a key: the list of set positions is wave-uniform and read through the constant address space (scalar loads).
//   * a * s is exact (integer adds over the set positions, mod 2^64, negacyclic) and defined once: negacyclic_key_product, shared by the row kind and the TRLWE phase
//     body.  The mask lives in LDS SIGN-EXTENDED over 2N entries, ext[i] = -a[i], ext[N + i] = a[i], so that (a * s)[x] = sum over set positions p of ext[N + x - p]:
//     one 8-byte LDS read and one 64-bit add per term, no select.  16 N bytes of LDS (32 KiB at N = 2048, 64 KiB at N = 4096).
//   * Randomness: masks AND noise from ChaCha20 under the installed keygen secret, one block per (row, coefficient): words 0 - 3 give the noise term exactly as
//     keygen_noise computes it, words 4 - 5 of the same block the mask word (low word first).  Nonce = (call index << 8) | kind with kind 6 (TLWE), 7 (TRLWE), 8 (TRGSW).
//     No word depends on the chunking or on the launch geometry: rows are numbered from first_row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keygen_kernels.h"   // NoiseKey, MOSFHET_QR, workgroup_sync()

namespace mosfhet {

// chacha20_uniforms' block with words 4 - 5 as well: u1, u2 = the two uniforms of the noise term, mask = words 4 - 5 (low word first)
__device__ __forceinline__ void chacha20_uniforms_mask(const NoiseKey &key, uint64_t counter, uint64_t nonce, uint64_t &u1, uint64_t &u2, uint64_t &mask) {
  const uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3], key.k[4], key.k[5], key.k[6], key.k[7],
                          (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)nonce, (uint32_t)(nonce >> 32)};
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; i++) x[i] = s[i];
#pragma unroll 2
  for (int r = 0; r < 10; r++) {
    MOSFHET_QR(x[0], x[4], x[8], x[12]); MOSFHET_QR(x[1], x[5], x[9], x[13]); MOSFHET_QR(x[2], x[6], x[10], x[14]); MOSFHET_QR(x[3], x[7], x[11], x[15]);
    MOSFHET_QR(x[0], x[5], x[10], x[15]); MOSFHET_QR(x[1], x[6], x[11], x[12]); MOSFHET_QR(x[2], x[7], x[8], x[13]); MOSFHET_QR(x[3], x[4], x[9], x[14]);
  }
  u1 = (uint64_t)(x[0] + s[0]) | ((uint64_t)(x[1] + s[1]) << 32);
  u2 = (uint64_t)(x[2] + s[2]) | ((uint64_t)(x[3] + s[3]) << 32);
  mask = (uint64_t)(x[4] + s[4]) | ((uint64_t)(x[5] + s[5]) << 32);
}

// the noise term of keygen_noise (same expression, same block) and the mask word of coefficient x of row `row`
__device__ __forceinline__ uint64_t client_noise_and_mask(const NoiseKey &key, uint64_t row, uint64_t x, double sigma, uint64_t &mask) {
  uint64_t a, b;
  chacha20_uniforms_mask(key, (row << 16) | x, key.nonce, a, b, mask);
  const double u1 = ((double)(a >> 11) + 0.5) * 0x1p-53, u2 = ((double)(b >> 11) + 0.5) * 0x1p-53;
  const double z = cos(6.283185307179586 * u1) * sqrt(-2.0 * log(u2)) * sigma;
  return (uint64_t)(int64_t)(18446744073709551616.0 * z);
}

// decode rule of the phase calls: msg_bits = 0 the phase itself, else the message of msg_bits bits nearest to it
__device__ __forceinline__ uint64_t client_decode(uint64_t phase, int msg_bits) {
  return msg_bits ? (phase + (1ull << (63 - msg_bits))) >> (64 - msg_bits) : phase;
}

// The exact negacyclic product of the mask in `ext` (sign-extended, see above) with the key: sink(x, (a * s)[x]) for every coefficient this thread owns, x = tid + j * 256
// (a workgroup has 256 threads).  entries: cnt words (value << 16) | position; binary: every value is 1 (adds only), else the generators' multiply path.
// From N = 1024 on a thread takes four coefficients per pass over the list: their LDS addresses differ by immediates, so an entry costs one address subtraction, and a
// scalar load of eight entries feeds 32 reads that are all in flight before the first add.  N = 256, 512: one coefficient per pass.
template <class Sink>
__device__ __forceinline__ void negacyclic_key_product(const uint64_t *ext, const int *entries, int cnt, int binary, int N, int tid, Sink sink) {
  constexpr int THREADS = 256;
  typedef const int __attribute__((address_space(4))) *const_ints_t;   // the key image is not written while a kernel runs: scalar loads (LutStep's idiom)
  const const_ints_t tab = (const_ints_t)entries;
  if (N < 4 * THREADS) {
    for (int x = tid; x < N; x += THREADS) {
      const uint64_t *base = ext + N + x;
      uint64_t acc = 0;
#pragma unroll 8
      for (int q = 0; q < cnt; q++) {
        const int e = tab[q];
        acc += base[-(e & 0xffff)] * (uint64_t)(int64_t)(e >> 16);
      }
      sink(x, acc);
    }
    return;
  }
  for (int x0 = tid; x0 < N; x0 += 4 * THREADS) {
    const uint64_t *base = ext + N + x0;
    uint64_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    if (binary) {
#pragma unroll 8
      for (int q = 0; q < cnt; q++) {
        const uint64_t *at = base - (tab[q] & 0xffff);
        const uint64_t w0 = at[0], w1 = at[THREADS], w2 = at[2 * THREADS], w3 = at[3 * THREADS];
        acc0 += w0; acc1 += w1; acc2 += w2; acc3 += w3;
      }
    } else {
#pragma unroll 8
      for (int q = 0; q < cnt; q++) {
        const int e = tab[q];
        const uint64_t *at = base - (e & 0xffff);
        const uint64_t v = (uint64_t)(int64_t)(e >> 16);
        const uint64_t w0 = at[0], w1 = at[THREADS], w2 = at[2 * THREADS], w3 = at[3 * THREADS];
        acc0 += w0 * v; acc1 += w1 * v; acc2 += w2 * v; acc3 += w3 * v;
      }
    }
    sink(x0, acc0); sink(x0 + THREADS, acc1); sink(x0 + 2 * THREADS, acc2); sink(x0 + 3 * THREADS, acc3);
  }
}

// kind 1: row r is a fresh TRLWE sample: a uniform, b = a * s + e (+ msg, l = 0).  l > 0: row r = sample * 2l + c * l + j of a TRGSW sample, m 2^(64 - (j+1) Bg_bit) added to
// coefficient e of component c AFTER b was formed from the plain mask; exponent mod 2N, X^N = -1 (trgsw_monomial_sample).
// kind 2: out[b][x] = decode(in[b].b[x] - (in[b].a * s)[x]): trlwe_phase word for word, no transform.
// One workgroup of 256 threads per row / sample; ext: 2N words of dynamic LDS.
__device__ __forceinline__ void client_ring_body(const ClientParams &p, const NoiseKey &nkey, uint64_t *ext) {
  const int N = p.N, tid = threadIdx.x;
  if (p.kind == 2) {
    const uint64_t *src = p.in + (size_t)blockIdx.x * 2 * N;
    uint64_t *dst = p.out + (size_t)blockIdx.x * N;
    for (int x = tid; x < N; x += 256) {
      const uint64_t ax = src[x];
      ext[x] = (uint64_t)0 - ax;
      ext[N + x] = ax;
    }
    workgroup_sync();
    const int msg_bits = p.msg_bits;
    negacyclic_key_product(ext, p.key, p.cnt, p.binary, N, tid, [&](int x, uint64_t as) { dst[x] = client_decode(src[N + x] - as, msg_bits); });
    return;
  }
  const size_t r = p.first_row + blockIdx.x;
  uint64_t *dst = p.out + (r - p.rows_first) * 2 * (size_t)N;
  int c = -1, e = 0;
  uint64_t val = 0;
  if (p.l > 0) {
    const int q = (int)(r % (size_t)(2 * p.l)), j = q % p.l;
    const size_t sample = r / (size_t)(2 * p.l);
    const int e_full = (p.exp ? p.exp[sample] : 0) & (2 * N - 1);
    const uint64_t h = (uint64_t)(int64_t)p.m[sample] << (64 - (j + 1) * p.Bg_bit);
    c = q / p.l;
    e = e_full & (N - 1);
    val = (e_full & N) ? (uint64_t)0 - h : h;
  }
  const uint64_t *msg = p.in ? p.in + r * (size_t)N : nullptr;
  for (int x = tid; x < N; x += 256) {
    uint64_t ax;
    uint64_t bx = client_noise_and_mask(nkey, r, (uint64_t)x, p.sigma, ax);
    ext[x] = (uint64_t)0 - ax;
    ext[N + x] = ax;
    if (msg) bx += msg[x];
    dst[x] = ax + ((c == 0 && x == e) ? val : 0);
    dst[N + x] = bx + ((c == 1 && x == e) ? val : 0);   // (this thread owns coefficient x in the product too: its own word, no barrier needed for it)
  }
  workgroup_sync();
  negacyclic_key_product(ext, p.key, p.cnt, p.binary, N, tid, [&](int x, uint64_t as) { dst[N + x] += as; });
}

// kind 3: TLWE sample r: out[i] = a_i (mask word of block x = i), out[n] = sum a_i s_i + e + msg with e the noise term of block x = 0.
// kind 4: out[b] = decode(in[b][n] - sum in[b][i] s_i): tlwe_phase word for word.
// One wavefront per sample; rows of n + 1 words are not 16-byte aligned: 8-byte accesses.  Integer sums are order-free: any reduction tree gives the same word.
__device__ __forceinline__ void client_lwe_body(const ClientParams &p, const NoiseKey &nkey) {
  const size_t r = p.first_row + blockIdx.x;
  const int lane = threadIdx.x, n = p.N;
  uint64_t acc = 0;
  if (p.kind == 4) {
    const uint64_t *src = p.in + r * (size_t)(n + 1);
    for (int x = lane; x < n; x += 64) acc += src[x] * (uint64_t)(int64_t)p.key[x];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) p.out[r] = client_decode(src[n] - acc, p.msg_bits);
    return;
  }
  uint64_t *dst = p.out + r * (size_t)(n + 1);
  for (int x = lane; x < n; x += 64) {
    uint64_t ax;
    const uint64_t e = client_noise_and_mask(nkey, r, (uint64_t)x, p.sigma, ax);
    dst[x] = ax;
    acc += ax * (uint64_t)(int64_t)p.key[x];
    if (x == 0) acc += e + p.in[r];
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) dst[n] = acc;
}

}  // namespace mosfhet
