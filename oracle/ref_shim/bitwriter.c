/* The eight bit-writer entry points of ref_shim/ogg/ogg.h, written for this project: one bit at a time into a growing, zeroed
   buffer.  endbyte/endbit is the position of the next bit; a started byte counts in oggpackB_bytes. */
#include <string.h>
#include "ogg/ogg.h"

static int bw_room(oggpack_buffer *b) {
  if (!b->buffer) return 0;
  if (b->endbyte + 1 >= b->storage) {
    long n = b->storage * 2;
    unsigned char *p = (unsigned char *)realloc(b->buffer, (size_t)n);
    if (!p) { free(b->buffer); memset(b, 0, sizeof(*b)); return 0; }
    memset(p + b->storage, 0, (size_t)(n - b->storage));
    b->buffer = p;
    b->storage = n;
  }
  b->ptr = b->buffer + b->endbyte;
  return 1;
}

static void bw_put(oggpack_buffer *b, unsigned long value, int bits, int msb_first) {
  int i;
  if (bits < 0 || bits > 32) return;
  for (i = 0; i < bits; i++) {
    unsigned bit = (unsigned)(value >> (msb_first ? bits - 1 - i : i)) & 1u;
    if (!bw_room(b)) return;
    if (b->endbit == 0) *b->ptr = 0;
    *b->ptr |= (unsigned char)(bit << (msb_first ? 7 - b->endbit : b->endbit));
    if (++b->endbit == 8) { b->endbit = 0; b->endbyte++; b->ptr++; }
  }
}

void oggpackB_writeinit(oggpack_buffer *b) {
  memset(b, 0, sizeof(*b));
  b->storage = 256;
  b->buffer = b->ptr = (unsigned char *)calloc((size_t)b->storage, 1);
}
void oggpackB_write(oggpack_buffer *b, unsigned long value, int bits) { bw_put(b, value, bits, 1); }
void oggpack_write(oggpack_buffer *b, unsigned long value, int bits) { bw_put(b, value, bits, 0); }
long oggpackB_bytes(oggpack_buffer *b) { return b->endbyte + (b->endbit + 7) / 8; }
void oggpackB_reset(oggpack_buffer *b) {
  if (!b->buffer) return;
  b->ptr = b->buffer;
  b->buffer[0] = 0;
  b->endbit = 0;
  b->endbyte = 0;
}
unsigned char *oggpackB_get_buffer(oggpack_buffer *b) { return b->buffer; }
void oggpackB_writeclear(oggpack_buffer *b) {
  free(b->buffer);
  memset(b, 0, sizeof(*b));
}
void oggpack_writeclear(oggpack_buffer *b) { oggpackB_writeclear(b); }
