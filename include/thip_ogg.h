/* thip_ogg.h -- the part of an Ogg demultiplexer a Theora player needs, written from RFC 3533
 * (the reference leans on libogg for this -- ogg_sync_* / ogg_stream_* in
 * examples/dump_video.c:365-470 -- and libogg is not part of this image).  It turns the bytes of
 * a physical Ogg bitstream into the packets of its logical streams:
 *   - page capture on "OggS", stream structure version 0, header-type flags (continued packet,
 *     first page, last page), 64-bit granule position, serial number, page sequence number;
 *   - CRC-32 of every page (polynomial 0x04c11db7, initial value 0, no reflection, no final xor);
 *     pages that fail it are skipped and capture resumes at the next "OggS";
 *   - lacing: segments of 255 continue a packet, a shorter one ends it; packets may span any
 *     number of pages; a page-sequence gap drops the packet that was being assembled;
 *   - multiplexed (interleaved) and chained logical streams: every packet comes with its serial
 *     number, the caller keeps the ones it wants.
 * Not a general libogg replacement: no seeking.
 *
 * The writer (thip_ogg_writer_*) makes the pages of one logical stream: lacing, sequence numbers, CRC, header flags.  Its page
 * rule: a packet with b_o_s set goes on a page of its own (the first page, flagged first-of-stream); a page is closed once its
 * body reaches 4096 bytes after a packet ends, when 255 segments are full (the packet goes on, flagged continued, on the next
 * page), after a packet with e_o_s set (that page is flagged last-of-stream), and on thip_ogg_writer_flush.  A page's granule
 * position is that of the last packet that ends on it, -1 if none does.
 */
#ifndef THIP_OGG_H
#define THIP_OGG_H
#include <stddef.h>
#include <stdint.h>

#include "theoradec_hip.h" /* ogg_packet */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct thip_ogg_reader thip_ogg_reader;

/* The reader borrows [data, data+size): it must stay valid until thip_ogg_close. */
thip_ogg_reader *thip_ogg_open_memory(const uint8_t *data, size_t size);
/* Reads the whole file into memory first (players stream; a test harness does not need to). */
thip_ogg_reader *thip_ogg_open_file(const char *path);
/* Next packet of any logical stream, in page order.  Returns 1 and fills *op (op->packet points
   into storage owned by the reader, valid until the next call) and *serialno; 0 at the end of
   the data; the fields b_o_s / e_o_s / granulepos / packetno follow libogg's conventions
   (granulepos is -1 except on the last packet that ends on a page). */
int thip_ogg_next_packet(thip_ogg_reader *r, ogg_packet *op, uint32_t *serialno);
/* Pages dropped so far because of a bad checksum or lost capture, and sequence gaps seen. */
void thip_ogg_stats(const thip_ogg_reader *r, int64_t *bad_pages, int64_t *gaps);
void thip_ogg_close(thip_ogg_reader *r);

typedef struct thip_ogg_writer thip_ogg_writer;
thip_ogg_writer *thip_ogg_writer_new(uint32_t serialno);
/* Adds a packet (bytes may be 0).  Returns 0, or -1: bad arguments, a first packet without b_o_s, a packet after e_o_s. */
int thip_ogg_writer_packetin(thip_ogg_writer *w, const ogg_packet *op);
/* Closes the page being filled, if it holds anything (a Theora stream flushes after its setup header). */
int thip_ogg_writer_flush(thip_ogg_writer *w);
/* The bytes of the pages completed since the previous call; valid until the next call on w. */
const uint8_t *thip_ogg_writer_pages(thip_ogg_writer *w, size_t *size);
void thip_ogg_writer_free(thip_ogg_writer *w);

#ifdef __cplusplus
}
#endif
#endif
