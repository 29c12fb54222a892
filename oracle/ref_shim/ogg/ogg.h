/* Stand-in for <ogg/ogg.h>, written for this project: only what a Theora codec library needs to compile without libogg -- the
   integer types, the allocation macros, the packet struct, and the eight bit-writer entry points of bitwriter.c.  No container
   code.  TEST INFRASTRUCTURE ONLY (oracle/ref.py). */
#ifndef THIP_REF_SHIM_OGG_H
#define THIP_REF_SHIM_OGG_H
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

typedef int16_t ogg_int16_t;
typedef uint16_t ogg_uint16_t;
typedef int32_t ogg_int32_t;
typedef uint32_t ogg_uint32_t;
typedef int64_t ogg_int64_t;
typedef uint64_t ogg_uint64_t;

#define _ogg_malloc malloc
#define _ogg_calloc calloc
#define _ogg_realloc realloc
#define _ogg_free free

typedef struct {
  long endbyte;
  int endbit;
  unsigned char *buffer;
  unsigned char *ptr;
  long storage;
} oggpack_buffer;

typedef struct {
  unsigned char *packet;
  long bytes;
  long b_o_s;
  long e_o_s;
  ogg_int64_t granulepos;
  ogg_int64_t packetno;
} ogg_packet;

/* most significant bit first */
void oggpackB_writeinit(oggpack_buffer *b);
void oggpackB_write(oggpack_buffer *b, unsigned long value, int bits);
long oggpackB_bytes(oggpack_buffer *b);
void oggpackB_reset(oggpack_buffer *b);
unsigned char *oggpackB_get_buffer(oggpack_buffer *b);
void oggpackB_writeclear(oggpack_buffer *b);
/* least significant bit first, on the same buffer */
void oggpack_write(oggpack_buffer *b, unsigned long value, int bits);
void oggpack_writeclear(oggpack_buffer *b);
#endif
