// mjh_decode_dev.h -- device code shared by the Huffman decoder's kernel files (mjh_decode.hip: sequential files, mjh_decode_prog.hip:
// progressive files): the bit reader, one Huffman symbol, where a block of a scan lies, the workgroup's scan into LDS
#ifndef MJH_DECODE_DEV_H
#define MJH_DECODE_DEV_H
#include <hip/hip_runtime.h>
#include "mjh_device.h"
#include "mjh_decode.h"

struct DecReader {
  const uint8_t *d;
  unsigned len;
  unsigned long long acc;   // the 6 data bytes from byte p >> 3 on (stuffed zeros removed), in the low 48 bits
  // the next 41+ bits at bit position p, left-aligned in 64 bits; bytes behind the segment's end read as zero
  __device__ __forceinline__ unsigned long long fetch(unsigned p)
  {
    unsigned idx = p >> 3;
    unsigned long long a = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const unsigned byte = idx < len ? (unsigned)d[idx] : 0u;
      a = (a << 8) | byte;
      idx += 1u + (byte == 0xFFu ? 1u : 0u);
    }
    acc = a;
    return a << (16 + (p & 7u));
  }
  // p + nbits (nbits <= 33) in the segment's byte numbering: a consumed 0xFF takes its stuffed zero along
  __device__ __forceinline__ unsigned advance(unsigned p, int nbits) const
  {
    const unsigned tot = (p & 7u) + (unsigned)nbits;
    const int nbytes = (int)(tot >> 3);
    unsigned bp = p >> 3;
#pragma unroll
    for (int i = 0; i < 5; i++)
      if (i < nbytes) bp += 1u + ((((unsigned)(acc >> (40 - 8 * i))) & 0xFFu) == 0xFFu ? 1u : 0u);
    return (bp << 3) | (tot & 7u);
  }
};

// one Huffman symbol at the top of w: its length in nb (jpeg_huff_decode jdhuff.c:455-492); a code no table entry exists for
// reads as symbol 0 of 16 bits and sets bad
__device__ __forceinline__ int dec_symbol(const MjhDecTable &T, unsigned long long w, int &nb, bool &bad)
{
  const unsigned e = T.look[(unsigned)(w >> 56)];
  if (e) { nb = (int)(e >> 8); return (int)(e & 0xFFu); }
  int l = 9;
  int code = (int)(w >> (64 - 9));
  while (l <= 16 && code > T.maxcode[l]) { l++; code = (int)(w >> (64 - l)); }
  if (l > 16) { nb = 16; bad = true; return 0; }
  nb = l;
  return (int)T.huffval[(code + T.valoff[l]) & 0xFF];
}

// where block b of MCU `mcu` of the scan lies: component-in-scan j, the block's index in the component's planes (-1: a dummy
// block) and its index in the scan-order DC-difference array of the component
struct DecWhere { int j; int blk; long long m; };
__device__ __forceinline__ DecWhere dec_locate(const MjhComp *lc, const MjhDecScan &sc, int mcu, int b)
{
  DecWhere w;
  int j = 0, t = b;
  long long doff = sc.diff_off;
  while (j < sc.ncomp - 1 && t >= sc.nb[j]) { t -= sc.nb[j]; doff += (long long)sc.nb[j] * sc.mcus; j++; }
  w.j = j;
  const MjhComp &cc = lc[j];
  if (sc.ncomp == 1) { w.blk = mcu < cc.nblk ? mcu : -1; w.m = doff + mcu; return w; }
  const int my = mcu / sc.mcus_per_row, mx = mcu - my * sc.mcus_per_row;
  const int by = t / cc.h, bx = t - by * cc.h;
  const int row = my * cc.v + by, col = mx * cc.h + bx;
  w.blk = (row < cc.hib && col < cc.wib) ? row * cc.wib + col : -1;
  w.m = doff + (long long)mcu * sc.nb[j] + t;
  return w;
}

// the workgroup's (image, scan): its descriptor and tables into LDS (every lane of a workgroup belongs to the same scan)
__device__ __forceinline__ void dec_load_scan(const MjhConst &C, const MjhDecBatch &B, int scan, MjhDecScan *sc, MjhDecTable *T, MjhComp *lc)
{
  const unsigned *src = reinterpret_cast<const unsigned *>(B.scans + scan);
  unsigned *dst = reinterpret_cast<unsigned *>(sc);
  for (unsigned i = threadIdx.x; i < sizeof(MjhDecScan) / 4; i += MJH_DEC_WG) dst[i] = src[i];
  __syncthreads();
  for (int t = 0; t < sc->ncomp; t++) {            // (t is uniform: the geometry comes through scalar loads)
    const unsigned *cs = reinterpret_cast<const unsigned *>(&C.c[sc->comp[t]]);
    unsigned *cd = reinterpret_cast<unsigned *>(lc + t);
    for (unsigned i = threadIdx.x; i < sizeof(MjhComp) / 4; i += MJH_DEC_WG) cd[i] = cs[i];
  }
  for (int t = 0; t < 2 * sc->ncomp; t++) {
    const int ti = (t & 1) ? sc->actab[t >> 1] : sc->dctab[t >> 1];
    const unsigned *ts = reinterpret_cast<const unsigned *>(B.tables + ti);
    unsigned *td = reinterpret_cast<unsigned *>(T + t);
    for (unsigned i = threadIdx.x; i < sizeof(MjhDecTable) / 4; i += MJH_DEC_WG) td[i] = ts[i];
  }
  __syncthreads();
}

// first byte of subsequence i of a segment: i * S, or the byte behind it when that one is the stuffed zero of an 0xFF
__device__ __forceinline__ unsigned dec_sub_start(const uint8_t *d, unsigned len, unsigned i, unsigned S)
{
  unsigned bp = i * S;
  if (i > 0 && bp < len && d[bp - 1] == 0xFFu && d[bp] == 0u) bp++;
  return bp;
}
__device__ __forceinline__ unsigned dec_sub_end_bits(unsigned len, unsigned i, unsigned nsub, unsigned S)
{
  return (i + 1 >= nsub) ? len * 8u : (i + 1u) * S * 8u;
}
#endif
