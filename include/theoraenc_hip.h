/* theoraenc_hip.h -- libtheora's encoder API (include/theora/theoraenc.h) for an encoder whose block work runs on the MI355X,
 * intra-only by default, with motion-compensated inter frames on request (TH_ENCCTL_THIP_SET_INTER_FRAMES, "Inter frames" below): the same function names, signatures, TH_ENCCTL_* numbers and TH_E* return codes, so a program written against
 * libtheoraenc that asks for nothing beyond a constant quality relinks against libtheora_hip.so.  The shared types (th_info,
 * th_comment, th_ycbcr_buffer, ogg_packet) come from theoradec_hip.h.
 *
 * What it is not, by default: every data packet is a key frame.  There is no mode decision, motion search or rate control by
 * default.  Bitrate mode is entered through TH_ENCCTL_SET_BITRATE after th_encode_alloc ("Bitrate mode" below); th_info.target_bitrate
 * != 0 at th_encode_alloc is refused (NULL).  Two-pass encoding goes through TH_ENCCTL_THIP_2PASS_OUT / _IN ("Two-pass" below;
 * libtheora's own requests 24 and 26 answer TH_EIMPL, their record format is not this one).  Custom Huffman codes are taken through TH_ENCCTL_SET_HUFFMAN_CODES
 * ("Huffman codes" below) and custom quantisation parameters through TH_ENCCTL_SET_QUANT_PARAMS ("Quantisation parameters" below); VP3
 * compatibility is not available (TH_EIMPL).  An all-key-frame stream is valid Theora; every decoder plays it.
 *
 * The bitstream, stated so that a restatement reproduces the packets byte for byte (tests/enc_ref.py does):
 *   - Setup header.  Loop-filter limits lflim[qi] = (31 * (63 - qi) + 31) / 63.  AC and DC scales fall geometrically,
 *     acscale[qi] = round(400 * (10/400)^(qi/63)), dcscale[qi] = round(200 * (10/200)^(qi/63)).  Three base matrices, by
 *     natural position (row r, column c): luma 16 + 3 (r + c) + (r c) / 4, chroma 18 + 5 (r + c), inter 16 + 2 (r + c) (used by
 *     inter frames only).  Each (qti, pli) has ONE quant range of size 63
 *     whose two ends are the same base matrix, so every quantiser step of spec 6.4.3 is max(qmin, min(scale[qi] bm / 100 * 4,
 *     4096)): non-increasing in qi.  80 Huffman trees: for Huffman group hg (0..4) and table t (0..15), t = 4 a + b, the
 *     Huffman code of 32 token weights with a sparsity s = {0.1, 0.3, 0.55, 0.8}[b] and a magnitude ratio q = {0.15, 0.35,
 *     0.55, 0.75}[a] (thip_encode.hip, enc_token_weights); every token has a code, none longer than 31 bits.  These built-in trees are
 *     the default; TH_ENCCTL_SET_HUFFMAN_CODES replaces them ("Huffman codes" below) and changes nothing else of the header.  (The
 *     header is the same with inter frames on; the inter matrices are then used.)  These limits, scales, matrices and ranges are the
 *     built-in quantisation parameters; TH_ENCCTL_SET_QUANT_PARAMS replaces them ("Quantisation parameters" below) and changes
 *     nothing of the trees.
 *   - Frame.  An intra frame with one qi, qi = quality (TH_ENCCTL_SET_QUALITY changes it from the next frame); no block qi.
 *   - Blocks.  In coded order, each 8x8 block is pixel - 128, oc_enc_fdct8x8, oc_enc_quantize with the intra table of (plane,
 *     qi).  Pixels outside the picture region take the value of the nearest picture pixel (clamped coordinates) in every plane;
 *     the chroma picture region is the one of spec 4.4.
 *   - DC.  The value coded is the quantised DC minus the spec 7.8 predictor of the quantised DCs of the left, upper-left,
 *     upper and upper-right neighbours, with its +-128 rule; a plane's first fragment predicts from 0.
 *   - Tokens of a block, for each non-zero coefficient after g >= 0 zeros: a combined token if one fits (RUN_CAT1A/B/C for +-1
 *     with 1 <= g <= 17, RUN_CAT2A/B for +-2, +-3 with 1 <= g <= 3); else, if g > 0, one zero-run token (SHORT_ZRL for g <= 8,
 *     else ZRL) and then the smallest value token.  An EOB ends a block whose last non-zero coefficient lies before index 63.
 *   - Token order is the decoder's (spec 7.7.3): index, then plane (Y, Cb, Cr), then coded order.  Maximal runs of consecutive
 *     EOBs in that order become EOB-run tokens, across lists and planes, in pieces of at most 4095, each with the smallest token
 *     that fits and placed in the list of its first EOB.
 *   - Huffman tables.  The four table indices (DC luma, DC chroma, AC luma, AC chroma) are those that minimise the frame's bits;
 *     on a tie the lower index.
 *   - A value the largest value token cannot carry (|v| > 580) counts as an overflow and th_encode_packetout returns TH_EFAULT.
 *     The minimum quantisers of spec 6.4.3 make this unreachable.
 *   - Granule positions are those th_decode_packetin reports for the same packets (bitstream 3.2.1 numbering): key frame n,
 *     counted from 0 with the duplicates, gets (n + 1) << shift, and the k-th duplicate after it ((n + 1) << shift) + k.
 *
 * Inter frames (TH_ENCCTL_THIP_SET_INTER_FRAMES), stated likewise (tests/enc_inter_ref.py restates them).  Coordinates are the
 * bitstream's (rows from the bottom), vectors in half pixels of luma.
 *   - Key frames are the frames above.  Frame n (counted from 0 with the duplicates) is a key frame when it is the first, when its
 *     offset from the last key frame is >= the interval N (TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE), or when that offset plus its
 *     own duplicates would reach 1 << keyframe_granule_shift; otherwise an inter frame.  Granules: frame n after key frame m gets
 *     ((m + 1) << shift) + (n - m).
 *   - Reference: PREV only, the decoder's picture of the previous frame (loop filter included; the encoder keeps it by decoding its
 *     own packets).  One qi, = quality; INTRA blocks use the intra tables, all others the inter tables of that qi (spec 6.4.3).
 *   - Motion search, per macro block on luma (16 x 16), reads of PREV clamped to the plane as the decoder's:
 *     full pel: every (dx, dy) in [-15, 15]^2 by SAD; the least of the key (SAD, 2 (|dx| + |dy|), (dy + 15) 31 + dx + 15).
 *     half pel: the eight vectors 2 (dx, dy) + (hx, hy), hx, hy in {-1, 0, 1}, predicted as the decoder predicts (the truncating
 *     average of the two reads of spec 7.9.4); with the centre, the least of (SAD, |mvx| + |mvy|, 3 (hy + 1) + hx + 1) gives Smv
 *     and (mvx, mvy).  S0 = the SAD of vector 0, SI = the sum over the four luma blocks of the SAD against the block's mean
 *     (sum + 32) >> 6.
 *   - Mode (per macro block, L = the inter luma step at zig-zag index 1): MV if Smv + L < S0, else NOMV with S = S0 (S = Smv for
 *     MV); then INTRA if SI + 4 L < S.  In coded order over the macro blocks that have a coded luma block, an MV vector equal to
 *     the last one written or reused becomes INTER_MV_LAST, equal to the one before INTER_MV_LAST2, else INTER_MV (spec 7.5.2's
 *     bookkeeping).  Chroma uses the macro block's vector as the decoder derives it (4:2:0, 4:2:2: quarter pels on a decimated axis).
 *   - Blocks: pixel minus prediction (128 for INTRA; PREV through the vector otherwise), clamped source as for key frames,
 *     oc_enc_fdct8x8, oc_enc_quantize.  Every block of an INTRA or MV macro block is coded; a block of a NOMV macro block is coded
 *     when a level is not zero, else uncoded (copied from PREV).  A macro block with no coded luma block writes no mode (it is
 *     INTER_NOMV to the decoder).  A frame with no coded block is a zero-byte packet (the decoder's duplicate).
 *   - DC: spec 7.8 with reference classes: a neighbour counts when coded and of the same class (intra, or PREV); with none, the
 *     last coded quantised DC of that class before the block in the plane's raster order (0 if none).
 *   - Header: 0, 1 (inter), qi, 0.  Coded flags (spec 7.3): partially coded super blocks, then of the others the fully coded
 *     ones (long runs), then the block flags of the partial ones (short runs; never longer than 30).  Modes (7.4): the scheme of
 *     fewest bits (scheme 0 costs 24 more; ties: the lower scheme); scheme 0's alphabet by falling frequency, ties to the lower mode.
 *     Vectors (7.5): scheme 1 (six bits a component) when it costs fewer bits than the VLC, else the VLC.  Tokens as for key frames,
 *     over the coded blocks only.
 *
 * All eight modes (TH_ENCCTL_THIP_SET_INTER_MODES with inter frames on), stated likewise (tests/enc_modes_ref.py restates them).  The
 * inter frames above with these differences; with GOLD and the per-block terms left out the rule is the one above.
 *   - References: PREV, and GOLD, the decoder's picture of the last key frame (the encoder's own decoder's THIP_FRAME_GOLD).
 *   - Search, per macro block on luma: S0, Smv, (mvx, mvy) and SI as above.  Per luma block b (the decoder's order: bottom left,
 *     bottom right, top left, top right), the same two stages on the 8 x 8 block against PREV: full pel over [-15, 15]^2 with the key
 *     (SAD, 2 (|dx| + |dy|), raster index), then the eight half-pel neighbours with (SAD, |mvx| + |mvy|, 3 (hy + 1) + hx + 1), giving
 *     Sb and (bx_b, by_b); S4 = the sum of the four Sb.  Against GOLD: G0 (vector 0), and Gmv, (gx, gy) by the macro block's two
 *     stages.
 *   - Mode (L as above): (1) the PREV choice above: NOMV with C = S = S0, or MV with C = Smv + L, S = Smv; (2) INTER_MV_FOUR if
 *     S4 + 4 L < C, then C = S4 + 4 L, S = S4; (3) CG = G0 + L (GOLDEN_NOMV), or GOLDEN_MV with CG = Gmv + 2 L if Gmv + 2 L < G0 + L;
 *     that golden mode if CG < C, with S = G0 or Gmv; (4) INTRA if SI + 4 L < S.  Ties keep the earlier choice, so no golden mode
 *     wins while GOLD is PREV (the frame after a key frame).
 *   - Blocks: GOLDEN_NOMV and GOLDEN_MV predict from GOLD through 0 or (gx, gy); INTER_MV_FOUR luma blocks through their own vectors,
 *     its chroma through the vector the decoder derives (spec 7.5.2: 4:2:0 the rounded average of the four, 4:2:2 of the row's two,
 *     4:4:4 the block's own).  Every block of an INTRA, MV, MV_FOUR, GOLDEN_NOMV or GOLDEN_MV macro block is coded; NOMV as above.
 *   - DC: three reference classes (intra, PREV, GOLD), each with its own last coded DC.
 *   - Modes and vectors: INTER_MV becomes INTER_MV_LAST / LAST2 as above; INTER_MV_FOUR writes its four vectors (block order) and
 *     then last2 = last1, last1 = the fourth; GOLDEN_MV writes its vector and leaves last1 and last2 alone.  The scheme choice is the
 *     one above over all eight modes.
 *
 * Block-level qi (TH_ENCCTL_THIP_SET_BLOCK_QI with a delta D in 1..31), stated likewise (tests/enc_bqi_ref.py restates it).  It applies to
 * key frames and to inter frames with five or eight modes, in quality and in bitrate mode; everything not named here is as above.
 *   - The frame's qi list: qis[0] = the frame's qi (the quality, or the controller's choice), then max(qis[0] - D, 0) (coarser) and
 *     min(qis[0] + D, 63) (finer); a value equal to one already in the list is left out, so nqis is 2 or 3.
 *   - Header (spec 7.1): after qis[0] a 1 and qis[1], then a 1 and qis[2] when nqis = 3, else a 0 (a key frame's 3 reserved bits follow).
 *   - The qii flags (spec 7.6), after the vectors of an inter frame or straight after the header of a key frame, before the tokens,
 *     over the coded blocks in coded order: one flag qii > 0 a block as long runs (7.2.1); then, when nqis = 3 and a block has
 *     qii > 0, one flag qii > 1 for each block with qii > 0, as long runs.
 *   - Dequantisation: the DC always at qis[0] (its quantiser, its prediction and the loop-filter limit are those above); the AC
 *     coefficients at qis[qii], through the intra or inter table of the block's plane.
 *   - The choice, per block: c = the fDCT of the block's residual under its mode (before the quantiser); for each k < nqis, with
 *     levels l_z = oc_enc_quantize(c_z) and steps s_z of the block's table at qis[k]:
 *       D_k = sum over z >= 1 of (c_z - l_z s_z)^2;
 *       R_k = the bits of the block's AC tokens: the tokens of the levels at z >= 1 as if the DC were not zero (the walk starts at
 *             index 1), and the block's own EOB when its last non-zero level lies before index 63 (or at index 1 when all are zero);
 *             each token costs its code length in the AC table of its start index's Huffman group for the block's plane (luma,
 *             chroma) plus its extra bits.  The AC table indices are those the previous packet of the same frame type (key, inter)
 *             chose; before there is one, 5;
 *       lambda = (s * s * 40) >> 7, s = the step at zig-zag index 1 of the block's table at qis[0] (about 0.31 s^2;
 *             high-rate theory's 0.115 s^2 let the real cost rise at quality 16);
 *       J_k = D_k + lambda R_k, plus lambda for k != 0 (a bit's worth against the flags), in 64-bit integers (no term overflows).
 *     The block takes the least J_k; on a tie the lower k.  Its DC is quantised at qis[0] whatever it takes.
 *   - Coded blocks in inter frames: a block of a NOMV macro block is coded when a level is not zero (the DC at qis[0], the AC at its
 *     chosen qi).
 *   - Bitrate mode: the probe is unchanged (it models one qi) and the controller chooses qis[0]; c_key and c_inter absorb the rest.
 *
 * Activity masking (TH_ENCCTL_THIP_SET_MASKING with a ratio k in 2..16), stated likewise (tests/enc_mask_ref.py restates it).  It
 * scales the lambda of the block-qi choice above per block by how well the block's texture hides quantisation noise (libtheora's
 * oc_mb_activity and oc_mb_masking, carried by the only channel the format has for it, the block's qi).  It acts where block qi
 * does and only with it; off (k = 0, the default) and with block qi off every packet is as without the call.  Integer arithmetic
 * throughout, 64-bit where a product needs it; every division rounds down.
 *   - Activity: for every luma fragment, a = oc_mb_activity's _activity value of the block (analyze.c:1152-1237: 64 x the block's
 *     variance, capped at 5 << 12 where it is under 8 << 12, and damped through the integer logarithm and exponential where one of
 *     the four directional edge energies holds more than 40 % of their sum -- thip_enc_mb_cost_maps' `activity`, theora_hip.h),
 *     computed over the frame-size luma plane obtained by extending the picture region with clamped coordinates: the source the
 *     block kernels code from.  Where the picture region is the whole frame it is thip_enc_mb_cost_maps of the input, value for
 *     value.  It is the activity of the source frame, for key and inter frames alike, whatever a block's mode.
 *   - Average: A = max(64, (sum of a + n / 2) / n) over the n luma fragments of the frame.
 *   - Luma scale, Q11: i = (2048 (k a + A) + (a + k A) / 2) / (a + k A); it lies in [2048 / k, 2048 k] and is 2048 at a = A.
 *   - Chroma scale: a chroma fragment belongs to the macro block that holds it.  With that macro block's four luma scales sorted,
 *     i0 <= i1 <= i2 <= i3: m = i0 if i0 >= 2048, else i1; the chroma scale is max(m, 2048) (the reference's rule: chroma's weight
 *     is never lowered, and one flat luma block is ignored).
 *   - Use: lambda_b = (lambda i_b + 1024) >> 11 replaces lambda in every J_k of the block, the term for k != 0 included.  It may
 *     be 0.  Nothing else changes: the qi list, the DC at qis[0], the flags, the mode decision's L, the rate probe and controller
 *     (c_key and c_inter absorb it), the automatic-key-frame measurement, the quality statistics, the device packetiser.
 *   - No wait: two launches (the activity, then the scales) are queued in front of the frame's block-qi kernel; A and the largest
 *     activity come back with the frame's other read-backs (thip_enc_mask_stats).
 *
 * Region of interest (TH_ENCCTL_THIP_SET_ROI_MAP), stated likewise (tests/enc_roi_ref.py restates it).  A caller's importance map
 * scales the lambda of the block-qi choice per block, alone or on top of activity masking's scale.  It acts where block qi does and
 * only with it; without a map, and with a map that is 0 everywhere, every packet is byte for byte as without the call.  Integer
 * arithmetic throughout; every division rounds down and every >> is arithmetic.
 *   - The map: v[Hm][Wm], int8, every entry in -64..64, row 0 the picture's top row; it covers th_info's picture region (pic_x,
 *     pic_y, pw = pic_width, ph = pic_height) exactly.  Wm and Hm each lie in 1..16384, whatever the picture's size: the map may be
 *     coarser or finer than pixels.  Positive means more important; the unit is 1/16 of an octave of lambda.
 *   - The cell of a luma pixel (x, y) in picture coordinates, rows from the top: x' = min(max(x, 0), pw - 1), y' = min(max(y, 0),
 *     ph - 1) -- the clamp the block kernels apply to the source --, and (cx, cy) = (x' Wm / pw, y' Hm / ph).
 *   - The sum of a fragment of plane p: S = the sum of v[cy][cx] over its 64 samples, the sample at plane coordinates (X, Y) (rows
 *     from the top of the frame) evaluated at the luma pixel ((X << hdec_p) - pic_x, (Y << vdec_p) - pic_y); the shifts are 0 for
 *     luma and the plane's decimation for chroma.  One rule for the three planes and the three pixel formats.
 *   - The exponent: e = (S + 32) >> 6, in -64..64; n = -e, o = n >> 4, f = n & 15.
 *   - The ROI scale, Q11: r = T[f] << o when o >= 0, else (T[f] + (1 << (-o - 1))) >> -o, with T[f] = round(2048 2^(f / 16)):
 *       T = 2048, 2139, 2233, 2332, 2435, 2543, 2656, 2774, 2896, 3025, 3158, 3298, 3444, 3597, 3756, 3922.
 *     r lies in [128, 32768] and is 2048 where the map is 0.
 *   - The fragment's scale: i_b = min(max((m_b r_b + 1024) >> 11, 128), 32768), m_b masking's scale of the fragment when masking is
 *     on, else 2048.
 *   - Use: i_b is the i_b of "Activity masking", of "Skip decision" and of "Level choice", wherever masking's scale is used.  Nothing
 *     else changes: the qi list, the DC at qis[0], the mode decision's L, the rate probe and controllers, the pass file, automatic key
 *     frames, the quality statistics, the device packetiser.
 *   - No wait: one kernel a lane a fragment and a one-group fold are queued in front of the frame's block-qi kernel, behind masking's
 *     launches; the frame's extremes come back with its other read-backs (thip_enc_roi_stats).
 *
 * Rate-distortion mode decision (TH_ENCCTL_THIP_SET_RD_MODES), stated likewise (tests/enc_rd_ref.py restates it).  It replaces the
 * cascade of SAD comparisons of "All eight modes" by the least D + lambda R over six candidates, computed from the quantised levels
 * and the token code lengths.  Off (the default) every packet is as without the call.  Integer arithmetic throughout, 64-bit where a
 * product needs it.
 *   - Where it acts: on inter frames with inter frames and all eight modes on; with eight modes off the request is accepted and does
 *     nothing.  It does not touch key frames, the search (S0, Smv, S4, G0, Gmv, SI and their vectors are those of "All eight modes"),
 *     the rate probe, the controller, the automatic-key-frame measurement, the coded-block rule, or anything after the macro-block
 *     words: block qi is chosen afterwards, as always, on the winning mode's residual.
 *   - Candidates, per macro block, in this order: 0 INTER_NOMV (PREV, vector 0); 1 INTER_MV (PREV, (mvx, mvy)); 2 INTER_MV_FOUR (the
 *     four block vectors, chroma through the vector the decoder derives); 3 GOLDEN_NOMV (GOLD, vector 0); 4 GOLDEN_MV (GOLD, (gx, gy));
 *     5 INTRA (pixel - 128).
 *   - Blocks of a macro block: its four luma blocks and the chroma fragments that belong to it: 1 + 1 (4:2:0), 2 + 2 (4:2:2),
 *     4 + 4 (4:4:4).
 *   - Per block b under candidate m: c = the fDCT of the residual under m (the clamped source exactly as the block kernels take it);
 *     l = oc_enc_quantize(c) with the table of (intra for INTRA, else inter; plane) at the frame's qi, qis[0]; s that table's steps;
 *       D_b = sum over all 64 z of (c_z - l_z s_z)^2;
 *       R_b = the bits of the block's tokens counted as the rate probe counts a block: the walk starts at index 0, with the block's
 *             own EOB; each token costs its code length in the table of its start index's Huffman group for the block's plane plus
 *             its extra bits (a value no value token carries, |v| > 580, costs the largest one).  For R_b only, the level at index 0
 *             is replaced by the charged DC d': d' = l_0 for the five inter candidates; for INTRA d' = l_0 for luma block 0 and for
 *             every chroma block, and l_0 less luma block 0's l_0 for luma blocks 1..3.  No prediction across macro blocks: the cost
 *             depends on nothing outside the macro block.
 *     The four tables (DC luma, DC chroma, AC luma, AC chroma) are those the previous inter packet chose; before there is one, 5.
 *     Exception, following the coded rule: under candidate 0 a block whose 64 levels are all zero is uncoded: R_b = 0 and
 *     D_b = sum c_z^2.
 *   - lambda = (s1 * s1 * 40) >> 7, s1 the inter luma step at zig-zag index 1 of the frame's qi (block qi's lambda; neither masking
 *     nor the search's L enters).
 *   - Header bits H_m for candidates 0..5: 1, 15, 55, 5, 18, 4 (a mode code plus six bits a component for each vector written, flat;
 *     LAST / LAST2 are a serial matter and stay with the packet writer).
 *   - J_m = sum over the blocks of (D_b + lambda R_b) + lambda H_m, in 64-bit integers.  The macro block takes the least J_m; on a
 *     tie the lower index, so while GOLD is PREV candidate 3 never wins.  The word written is k_enc_me_all's, field for field.
 *   - No wait: two launches (the candidates, then the choice) stand in for the search's one (thip_enc_rd_stats).
 *
 * Skip decision (TH_ENCCTL_THIP_SET_RD_SKIP), stated likewise (tests/enc_skip_ref.py restates it).  After a block has been coded it
 * asks whether leaving it uncoded -- the decoder then keeps PREV's pixels there -- would have cost less (libtheora's oc_skip_cost,
 * analyze.c:829-867).  Off (the default) every packet is as without the call.  Integer arithmetic throughout, all of it 64-bit.
 *   - Where it acts: on inter frames, with five or eight modes, with or without block qi, masking, the rate-distortion mode decision,
 *     bitrate mode, two-pass, automatic key frames, the device packetiser and the quality statistics.  It does not touch key frames,
 *     the search, the mode decision (the SAD cascade or the rate-distortion one), the rate probe, the controllers (c_inter absorbs
 *     it) or the automatic-key-frame measurement.  With inter frames off the request is accepted and does nothing.
 *   - Which blocks: every block the rules above would code (any block of an INTRA, MV, MV_FOUR or golden macro block; a block of an
 *     INTER_NOMV macro block with a level that is not zero), except the luma blocks of an INTER_MV_FOUR macro block: an uncoded luma
 *     block there changes the vectors the decoder derives (spec 7.5.2).
 *   - Per block, after the block-qi choice k (k = 0 with block qi off), with c the fDCT of the block's residual, l its levels and s
 *     the steps of its table -- the DC (z = 0) at qis[0], the AC at qis[k]:
 *       D_code = sum over all 64 z of (c_z - l_z s_z)^2;
 *       R      = block qi's R_k: the AC tokens from index 1 with the block's own EOB, counted with the AC tables the previous inter
 *                packet chose (5 before there is one);
 *       lambda_b = block qi's lambda, (s1 * s1 * 40) >> 7 with s1 the step at zig-zag index 1 of the block's table at qis[0], and
 *                where masking acts (block qi and masking on) (lambda i_b + 1024) >> 11;
 *       SSD    = sum over the block's 64 pixels of (source - PREV at the same position)^2, the source clamped outward exactly as the
 *                block kernels read it;
 *       D_skip = 16 SSD, doubled when the vector the block is predicted through -- the vector of its plane that follows from the
 *                macro block's word, for an MV_FOUR chroma block the one the decoder derives -- is not (0, 0) (the reference's
 *                coded_ssd <<= 4 and its doubling, analyze.c:2008-2012).
 *     The block is left uncoded when D_skip <= D_code + lambda_b R.
 *   - Luma is decided first.  A macro block whose four luma blocks all end uncoded writes no mode and is INTER_NOMV to the decoder.
 *     Its chroma blocks are then coded as INTER_NOMV blocks whatever the macro block's word says: the residual against PREV at
 *     vector 0 through the inter tables, class PREV, coded when a level is not zero and the test (not doubled) does not leave the
 *     block out.  The chroma blocks of every other macro block follow the word as ever, then the test.
 *   - A frame with no coded block is the zero-byte packet, as ever.
 *   - No wait: two launches (the luma blocks, then the chroma blocks) stand in for the quantising kernel's one (thip_enc_skip_stats).
 *
 * Level choice (TH_ENCCTL_THIP_SET_RD_QUANT = w), stated likewise (tests/enc_rdq_ref.py restates it).  After the frame's blocks have
 * been quantised -- every level oc_enc_quantize(c), round to nearest -- it asks of each coded block which of its AC levels are worth
 * their tokens (libtheora's oc_enc_tokenize_ac, tokenize.c:457-744, decides the same question).  Off (w = 0, the default) every packet
 * is as without the call.  Integer arithmetic throughout, all of it 64-bit.
 *   - Where it acts: on every coded block of every frame: all blocks of a key frame; on an inter frame the blocks with a coded flag,
 *     after the mode decision, the block-qi choice and the skip decision, all three of which are made on the plain levels as ever.
 *     With five or eight modes, block qi, masking, the rate-distortion mode decision, the skip decision, bitrate mode and two-pass (the
 *     probe is unchanged; c_key and c_inter absorb it), automatic key frames, the device packetiser, the quality statistics, RGB and
 *     device input.  It changes AC levels (z >= 1) of coded blocks only: never the DC, the block's qii, a coded flag, a mode or a
 *     vector.  A block whose AC levels all become zero stays coded (an EOB at its first index).
 *   - Per block: c the fDCT of the block's residual under the mode it was coded with (the chroma of a macro block none of whose luma
 *     blocks is coded: against PREV at vector 0, as "Skip decision" has it); l its levels as the quantising kernel left them, the AC at
 *     qis[k] of the block's qii k; s the steps of its table at qis[k].
 *   - Candidates at z = 1..63: a level 0 stays 0; |l_z| = 1 may stay or become 0; |l_z| >= 2 may stay or become l_z - sgn(l_z).
 *     a_z = 0 names the original, a_z = 1 the alternative; l' the levels under a.
 *   - J(a) = sum over z >= 1 of (c_z - l'_z s_z)^2 + lambda_q R(l'), with R block qi's R_k: the AC tokens of l' from index 1 with the
 *     block's own EOB, each its code length in the AC table of its start index's Huffman group for luma or chroma plus its extra bits,
 *     the tables those the previous packet of the same frame type chose (5 before there is one); and lambda_q = (lambda_b w) >> 4
 *     with lambda_b the block's lambda of "Skip decision": (s1 * s1 * 40) >> 7 from its table at qis[0], and where masking acts
 *     (lambda i_b + 1024) >> 11.
 *   - The block takes the a of least J(a); among those the first in lexicographic order of (a_1, ..., a_63): it rather keeps an earlier
 *     coefficient as it is.  With lambda_q = 0 the block is left as it is (what the least J gives for levels rounded to nearest).
 *     The minimum is exact: a level with |l| >= 2 stays non-zero under both candidates, so a backward programme over the non-zero
 *     positions finds it -- F[i] the least cost of everything behind a kept position i, over the next kept position up to and
 *     including the first with |l| >= 2, or over the block's EOB when only +-1 remain.
 *   - No wait: one launch behind the frame's quantising (or skip) launches, in front of the DC and token kernels
 *     (thip_enc_rd_quant_stats).
 *
 * Bitrate mode (TH_ENCCTL_SET_BITRATE), stated so that a restatement reproduces the choices (tests/enc_rate_ref.py does).  Integer
 * arithmetic throughout; x >> 16 of a product is an arithmetic shift.
 *   - The probe.  Before a frame is coded (key or inter by the rule above), the device measures E[q], q = 0..63: the frame's bits
 *     at qi q counted from its tokens with every block's EOB its own token (no EOB runs).  Each token is counted in the list of the
 *     zig-zag index where it starts, in the Huffman group of that index, for luma or chroma; per choice (DC luma, DC chroma, AC luma,
 *     AC chroma) the least, over the 16 tables, of sum count x code length (for AC one table over groups 1-4), plus the tokens'
 *     extra bits, plus the header: 28 bits for a key frame, 25 + nfrags / 8 for an inter frame.  A key frame's blocks are the
 *     bitstream's at q.  An inter frame's macro-block mode at q follows from the search's S0, Smv, SI and vector with L = the inter
 *     luma step of q (the mode rule above); each block codes its macro block's residual at q and is coded by the rule above, exact
 *     except: (1) a DC is predicted from the coded neighbours of its class at q, and with none from 0; (2) instead of the coded
 *     flags, modes and vectors, 3 M(q) + 12 V(q) bits, M(q) the macro blocks with a coded luma block, V(q) those of them MV.
 *   - Setup, at the first frame in bitrate mode: T = clamp(bitrate * fps_denominator / fps_numerator, 32, 2^40) bits a frame;
 *     D = the buffer (TH_ENCCTL_SET_RATE_BUFFER), else clamp(K, 12, 256) with K the key-frame interval in force (1 with inter frames
 *     off); R = T D, F* = R / 2, fullness F = F*.  Per frame type t (key, inter) a correction c_t = 65536 (Q16) and the type's last
 *     probe L_t (none yet).
 *   - Each frame n (not a duplicate): L_t = E; Cur(q) = E[q] c_t >> 16.  Of frames n + 1 .. n + D - 1, n_k are key frames and
 *     n_i inter frames by the interval rule from the current key position (all key frames with inter frames off);
 *     Future(q) = n_k (L_key[q] c_key >> 16) + n_i (L_inter[q] c_inter >> 16), where a missing inter term is the key term / 4 and a
 *     missing key term 4 x the inter term.  S = F + D T - F*.  qi = the largest q with Cur(q) + Future(q) <= S, else 0.
 *   - Drop: with TH_RATECTL_DROP_FRAMES, when the frame is not the first, F + T - Cur(0) < 0 and a duplicate's granule fits there
 *     (frame offset from the key frame plus the frame's own duplicates < 1 << keyframe_granule_shift), the frame becomes a zero-byte
 *     packet with a duplicate's granule: F += T, the reference is unchanged, and it counts as a frame for the key-frame rule.
 *   - After a coded frame of A bits (8 x its bytes): F += T - A; c_t = clamp((c_t + (A << 16) / max(E[qi], 1)) / 2, 4096, 2^20).
 *     A duplicate (TH_ENCCTL_SET_DUP_COUNT) adds F += T.  After every change of F: with TH_RATECTL_CAP_OVERFLOW F = min(F, R), with
 *     TH_RATECTL_CAP_UNDERFLOW F = max(F, 0).
 *   - A later TH_ENCCTL_SET_BITRATE recomputes T, R and F*, keeps D, and sets F = min(F, R); TH_ENCCTL_SET_RATE_BUFFER likewise
 *     with the new D.
 *   - The wait: in bitrate mode th_encode_ycbcr_in and TH_ENCCTL_THIP_YCBCR_IN_DEVICE queue the probe, wait on the host for its
 *     512 bytes, choose, and then queue the frame's launches at the chosen qi exactly as quality mode does at that qi (with inter
 *     frames, its own motion search with that qi's lambda).  Quality mode never waits, except for a frame measured for an automatic key frame
 *     ("Automatic key frames" below).
 *   - With all eight modes on, the probe is unchanged (E[q] models the five modes above); the frame is coded with the eight-mode
 *     search at the chosen qi, and c_inter absorbs the difference.
 *
 * Automatic key frames (TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES with a ratio t in 1..4096), stated so that a restatement reproduces every
 * choice (tests/enc_cut_ref.py does).  The interval N of "Inter frames" becomes a maximum: a frame that prediction no longer serves
 * starts a new key frame.  Off (t = 0, the default), every packet is as without the call.  The headers do not change.
 *   - When a frame is measured: when it is not a duplicate and the interval rule of "Inter frames" makes it an inter frame.  A frame
 *     that rule makes a key frame is not measured; with inter frames off no frame is.
 *   - What is measured: per macro block, against PREV, S0, Smv and SI of the five-mode search of "Inter frames" (this search also
 *     with all eight modes on).  Over all nmbs macro blocks of the frame, in 64-bit integers: P = sum min(S0, Smv), I = sum SI,
 *     N = the macro blocks with SI < min(S0, Smv).  N is reported only.
 *   - Decision: the frame is a key frame when 256 P >= t I and P >= 4 * 256 nmbs.  The second condition is a mean absolute
 *     prediction error of at least 4 levels a luma pixel: it keeps flat, noisy pictures (P about I, both small) from turning into
 *     all-key streams.  Neither depends on qi, so quality mode and bitrate mode decide alike.  Recommended t: 230 (P / I >= 0.9).
 *   - A cut key frame is a key frame in every respect: its granule, GOLD, the interval (it restarts from the frame),
 *     thip_enc_inter_stats.key, thip_enc_rate_stats.key.
 *   - Bitrate mode: the decision precedes the probe, which is then the key or the inter probe accordingly; the controller's key
 *     position for Future(q) is the frame itself, as for an interval key frame.  The drop rule is unchanged, and a dropped frame is
 *     not a key frame whatever was measured (thip_enc_cut_stats.cut is 0 for it).
 *   - The wait: a measured frame waits on the host for 32 bytes (P, I, N) before its launches are queued, in th_encode_ycbcr_in or
 *     TH_ENCCTL_THIP_YCBCR_IN_DEVICE.  A measured frame that stays an inter frame is coded from the statistics already on the
 *     device where they determine it: with five modes its macro-block words follow from them and the frame's lambda (one search
 *     a frame, in bitrate mode too, whose inter probe also reads them); with all eight modes the eight-mode search runs as
 *     always and the measurement is an extra search.
 *
 * Device packetiser (TH_ENCCTL_THIP_SET_DEVICE_PACK).  By default the host makes the token part of a packet: it reads the frame's
 * tokens back, merges the EOB runs, chooses the four Huffman tables and writes the bits.  With the packetiser on, the device does
 * those three steps by the same rules (runs cut into pieces of 4095 from their start and counted in the list of their first token;
 * per choice the table 0..15 of least sum count x code length, a tie to the lower index; MSB-first bits, the last byte padded with
 * zeros) and the host writes only the frame header, coded flags, modes, vectors and qii flags in front.  It changes no bit of any
 * packet, and nothing that follows from one (statistics, the rate controller's A, the block-qi tables, the reconstruction).  A frame
 * whose bits exceed the device's packet buffer (128 bytes a block) is packed by the host as by default and counted in
 * thip_enc_pack_stats.fallbacks.  The packet th_encode_packetout returns then lies in pinned host memory owned by the context, valid
 * as always until the next call on it.
 *
 * R'G'B' input (TH_ENCCTL_THIP_RGB_IN).  The request takes the picture as R'G'B' pixels, in host or in device memory, and does what
 * th_encode_ycbcr_in does for the picture-sized Y'CbCr planes thip_picture_in makes of them (theora_hip.h states the arithmetic: an
 * integer matrix, chroma the mean of the 1 << (hdec + vdec) pixels a sample covers with the picture's edge repeated), pic_x, pic_y
 * and the pixel format taken from the context's th_info.  The conversion runs on the device into an encoder-owned buffer, and every
 * mode above -- key and inter frames, eight modes, block qi, bitrate mode's probe, the automatic-key-frame measurement, the device
 * packetiser -- reads the converted planes as it reads any other input: the stream is a function of the R'G'B' bytes alone
 * (tests/picture_in_ref.py restates the conversion).
 *
 * Quality statistics (TH_ENCCTL_THIP_SET_QUALITY_STATS / _GET_QUALITY_STATS).  With the switch on the encoder says how good each
 * packet is: the packet goes through the encoder's own decoder (the one inter frames use; with inter frames off it now runs too),
 * and th_encode_packetout queues one thip_picture_compare (theora_hip.h states the sums and the integer SSIM) on the encoder's
 * stream: the decoder's newest picture over th_info's picture region against the source planes, which stay in the encoder's input
 * buffer until the next frame comes in.  TH_ENCCTL_THIP_YCBCR_IN_DEVICE therefore first copies the picture region into that buffer,
 * inside the ordering window the call has anyway, and the frame is coded from the copy: the caller may still overwrite its planes
 * as soon as the call returns.  A frame the rate controller dropped is measured against the picture a decoder goes on showing
 * (measured = 1); a TH_ENCCTL_SET_DUP_COUNT duplicate has no source (measured = 0, every sum 0).  The numbers are those a caller
 * gets who decodes the packets and sums (source - decoded)^2 over the picture region, the reference's dump_psnr among them.  The
 * switch changes no bit of any packet in any mode.
 *
 * Two-pass (TH_ENCCTL_THIP_2PASS_OUT, TH_ENCCTL_THIP_2PASS_IN), stated so that a restatement reproduces every byte and every choice
 * (tests/enc_2pass_ref.py does).  A first pass writes down, per packet, the curve E[0..63] the rate probe measured for the frame; a
 * second pass reads the whole file's curves and spends the file's bits at the most even qi that fits.
 *   - The pass file, little-endian throughout: a header of 1084 bytes, then one record of 264 bytes a packet, in packet order.
 *     Header: the magic "THP2" (bytes 0x54 0x48 0x50 0x32), u32 version = 1, then eleven u32: frame_width, frame_height, pic_x,
 *     pic_y, pic_width, pic_height, pixel_fmt, fps_numerator, fps_denominator, keyframe_granule_shift, the inter-frame switch (0 / 1);
 *     u32 frames (the records that are not duplicates), u32 duplicates (the records of type 2); then Tot[0][0..63] and Tot[1][0..63]
 *     as u64: per class (0 key, 1 inter) the sums of the records' E[q].  The placeholder the first call returns is the header with
 *     frames, duplicates and the sums 0.
 *     Record: u8 type (0 key, 1 inter, 2 a TH_ENCCTL_SET_DUP_COUNT duplicate, 3 a frame the rate controller dropped), u8 qi (the
 *     frame's qis[0]; for types 2 and 3 the last frame's), u16 0, u32 the packet's bits (saturating), E[0..63] as u32, each
 *     min(E[q], 2^32 - 1) (type 2: all 0).  A record's class: its type for 0 and 1; a dropped frame counts as class 1 with inter
 *     frames on, else 0; a duplicate has none and enters no sum.
 *   - Pass 1 changes no bit of any packet, in quality mode or in bitrate mode.  Every frame that is not a duplicate gets the probe
 *     of "Bitrate mode" against the reference it is really coded from, with the type it really has (interval rule, or a cut by
 *     automatic key frames).  In bitrate mode that probe runs anyway.  In quality mode its launches are queued on the encoder's
 *     stream in front of the frame's, the 512 bytes are copied asynchronously and read in th_encode_packetout: th_encode_ycbcr_in
 *     still never waits.
 *   - Pass 2 (bitrate mode only) is a controller of its own beside the one above.  N = frames + duplicates of the header, T as in
 *     "Bitrate mode" from the bitrate in force, B = T N, A = the bits of the packets so far; c_key = c_0, c_inter = c_1 as above; per
 *     class the recorded and the fresh curves of the frames so far, Seen[2][64] = Fresh[2][64] = 0.
 *   - Frame n (counted with the duplicates) needs record n.  Its type comes from the record: a key frame when the record's type is 0,
 *     an inter frame when it is 1; the interval rule and the cut measurement are not consulted.  Whatever the record says the frame
 *     is a key frame when it is the first, when inter frames are off, or when its offset from the last key frame plus its own
 *     duplicates reaches 1 << keyframe_granule_shift (with the same duplicates pass 1 decided the same).  Where the caller submits a
 *     frame whose record is a drop or a duplicate, it is coded as an inter frame under the same conditions; no frame is dropped in
 *     pass 2.  The caller repeats its own TH_ENCCTL_SET_DUP_COUNT calls: a duplicate packet consults no record and adds nothing to A.
 *   - The probe of "Bitrate mode" gives the fresh E.  The record's class t' (if it has one): for all q, Seen[t'][q] += Rec[q] and
 *     Fresh[t'][q] = min(Fresh[t'][q] + E[q], 2^62).  With t the frame's own type, Cur(q) = E[q] c_t >> 16.  Per class u,
 *     X = max(Tot[u][q] - Seen[u][q], 0), what the recorded curves leave; Y = X where Seen[u][q] = 0, else
 *     min(X Fresh[u][q] / Seen[u][q], 2^62) (128-bit product, the division rounding down): the rest of the file is taken to relate
 *     to its records as the fresh curves so far do to theirs, which absorbs the second pass's different reference; Future(q) = the
 *     sum over u of (Y c_u >> 16), c absorbing the flags, modes and vectors as in "Bitrate mode".  qi = the largest q with
 *     Cur(q) + Future(q) <= B - A, else 0.
 *   - After the packet of A_n bits: A += A_n, and c_t as in "Bitrate mode".  (A second Q16 correction per class averaged in after
 *     each packet, r = (r + A_n / Rec[qi]) / 2, was tried first: it learns a frame later and from one qi only, and landed farther
 *     from B; DESIGN.md section 5.17 has the figures.)
 *   - TH_ENCCTL_SET_RATE_FLAGS and TH_ENCCTL_SET_RATE_BUFFER are accepted in pass 2 and have no effect (there is no buffer and no
 *     drop).  thip_enc_rate_stats in pass 2: qi, key, target, estimate, actual, probe, corr as above; fullness_before, spend =
 *     B - A before the packet, fullness_after = B - A after it.  Block qi, masking, RD modes, the device packetiser and the quality
 *     statistics compose as with bitrate mode: the controller chooses qis[0].
 *
 * Huffman codes (TH_ENCCTL_SET_HUFFMAN_CODES, TH_ENCCTL_THIP_GET_TOKEN_HIST, thip_huff_train), stated likewise (tests/enc_huff_ref.py
 * restates them).  The 80 code sets are data to everything that counts or writes token bits: both packers, the block-qi choice, the
 * rate-distortion mode, skip and level decisions and the rate probe read the code lengths in force, so a caller's codes change their
 * prices with them; the rules above ("the table of least bits", "before there is one, 5") stay as stated.  With the same levels a
 * different code set gives the same pictures: the codes are lossless.
 *   - A code set is valid when every one of the 32 tokens has a code of 1..32 bits and the 32 codes form a full, prefix-free binary
 *     code (what libtheora's oc_huff_codes_pack accepts; a full code of 32 leaves is at most 31 deep); bits of `pattern` above `nbits`
 *     are ignored.  The setup header's tree of a set is then a function of its codes: pre-order, the 0 branch first.
 *   - The histogram of a packet (thip_enc_token_hist): the packet's merged tokens -- after the EOB runs are merged, what the packet
 *     holds -- counted per Huffman group of the list the token stands in (index 0; 1..5; 6..14; 15..27; 28..63), luma or chroma, and
 *     token.  It is the histogram the packer chooses the packet's four tables from, whichever packer made the packet.
 *   - thip_huff_train(hists, n, start, rounds, out, stats).  Samples: each histogram gives, for each class c (0 luma, 1 chroma), a DC
 *     sample count[0][c] and an AC sample count[1..4][c]; a sample whose counts are all 0 is dropped.  The samples are kept in the
 *     order packet, class, DC before AC.  DC and AC are trained apart, 16 tables each: DC table t is set t, AC table t the sets
 *     16 hg + t for hg = 1..4.
 *     Cost of a sample under table t: the sum of count x code length over its group or groups (the extra bits do not depend on the
 *     table and are left out).  Assignment: every sample goes to the table of least cost, on a tie the lower index (the packet
 *     writer's rule); the total cost is the sum of those least costs.
 *     Rebuild: for a table with at least one sample, and each group it covers, H[tok] = the sum of its samples' counts; the set
 *     becomes the Huffman code of the 32 weights 1024 H[tok] + 1 by the rule of the built-in trees: always merge the two lightest
 *     nodes, ties to the lower node id (leaves are 0..31, internal nodes are numbered from 32 in creation order), child 0 (code bit 0)
 *     the lighter of the two.  A table with no sample keeps its codes.
 *     Loop: the codes are `start` (patterns masked to nbits), B = the total cost of the assignment under them.  Up to `rounds` times:
 *     rebuild from the current assignment, assign anew under the rebuilt codes, giving B'; if B' < B the rebuilt codes, the new
 *     assignment and B = B' are accepted, otherwise the loop stops and the codes stay.  So bits_end <= bits_start always.  All sums
 *     are unsigned 64-bit and wrap; they are exact while the counts of all histograms together stay below 2^49.
 *     Empty tables are not reseeded or split: a pool whose samples all prefer a few tables trains those few.
 *
 * Quantisation parameters (TH_ENCCTL_SET_QUANT_PARAMS, TH_ENCCTL_THIP_GET_QUANT_PARAMS, thip_quant_info_from_setup), stated likewise
 * (tests/enc_quant_ref.py restates them).  The setup is data to everything that reads a step: every quantiser table, on the host
 * and on the device, is spec 6.4.3's over the parameters in force and is made at the first frame that needs it, so with a
 * caller's parameters every rule above holds as stated, with "the step" read from them.
 *   - A parameter set is valid when, for every (qti, pli), nranges is 1..63, sizes and base_matrices are not NULL, every size is
 *     >= 1 and the sizes sum to exactly 63; and no loop-filter limit is above 127 (the header's 3 bits of width carry at most 7 bits
 *     a limit).  Everything else is legal, as it is to a decoder: any 16-bit scale, 0 included, and any base-matrix byte -- qmin of
 *     spec 6.4.3 bounds every step from below (and 4096 from above), so the overflow rule (|v| > 580) stays unreachable; the
 *     TH_EFAULT path is kept.  libtheora trusts the caller; this library checks.
 *   - The setup header's quantiser part under a caller's parameters is what libtheora's oc_quant_params_pack writes.  Limits:
 *     3 bits of width w = ilog(the largest limit), then 64 x w bits.  AC scales, then DC scales: 4 bits of w - 1 with w =
 *     max(1, ilog(the largest scale)), then 64 x w bits.  The base matrices are consolidated by content, in first-seen order over
 *     (qti, pli, range end 0..nranges): 9 bits of their count - 1 (at most 384), then 64 bytes each; an index takes ilog(count - 1)
 *     bits, none when there is one matrix.  The six (qti, pli), intra Y, Cb, Cr then inter Y, Cb, Cr: the first writes its ranges;
 *     each later one writes, tested in this order, "01" when qti > 0 and its ranges (count, sizes, consolidated indices) equal
 *     those of (qti - 1, pli); "0" (qti = 0) or "00" (qti > 0) when they equal those of the (qti, pli) before it in that order; else
 *     "1" and its ranges.  Ranges: the index of the first matrix, then for each range its size - 1 in ilog(62 - the qi steps
 *     written so far) bits and the index of the matrix at its end.  The 80 trees follow unchanged.
 *   - The built-in header is NOT written this way: each of its six (qti, pli) states its ranges (the "1"), and it stays byte for
 *     byte what it was.  A caller who passes a copy of the built-in values (what TH_ENCCTL_THIP_GET_QUANT_PARAMS returns before any
 *     SET) gets a header that differs from the built-in one in those few bits, and the same pictures.  buf = NULL restores the
 *     built-in header itself.
 *   - lambda[qi], the weight of the motion search and, through it, of block qi, the RD modes, skip and the level choice, is the
 *     inter luma step at zig-zag index 1 at qi under the parameters in force.  The loop-filter limit of a frame is the
 *     parameters' limit at its qis[0].  The encoder's own decoder is set up from the header in force.
 *   - Block qi's list ("Block qi") goes by INDEX: qis[0] +- delta.  With scales that do not fall with qi, "coarser" and "finer" are
 *     only names for the lower and the higher index; the choice is still the least D + lambda R over the list.
 *   - Bitrate mode: the probe measures E[q] under the parameters in force at every q; E need not fall or rise with q, and the
 *     controller's choice is as stated, the LARGEST q whose estimate fits.  The probe's kernels walk, for each block, the indices
 *     whose coefficient is not zero under the least step over q of its (table, index): a superset at every q whatever the order of
 *     the steps.
 *   - Two-pass: the pass file's header does not carry the quantisers.  Both passes must be given the same ones, as for the
 *     Huffman codes; a second pass under other quantisers reads curves that are not its own.
 *
 * Device memory is allocated at the first th_encode_ycbcr_in (or TH_ENCCTL_THIP_YCBCR_IN_DEVICE / _RGB_IN / TH_ENCCTL_THIP_GET_DEVICE):
 * th_encode_alloc, th_encode_flushheader and th_encode_ctl with the libtheoraenc requests never touch the GPU; of the 0x72xx
 * extensions, YCBCR_IN_DEVICE, RGB_IN, GET_DEVICE and GET_QUALITY_STATS do.
 */
#ifndef THEORAENC_HIP_H
#define THEORAENC_HIP_H
#include "theoradec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* theoraenc.h control codes (same numbers).  Honoured: */
#define TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE (4) /* buf = ogg_uint32_t (4 bytes): accepted, 1 written back (with inter
                                                      frames on: TH_ENCCTL_THIP_SET_INTER_FRAMES) */
#define TH_ENCCTL_GET_SPLEVEL_MAX (12)             /* buf = int: 0 */
#define TH_ENCCTL_SET_SPLEVEL (14)                 /* buf = int: 0 only, else TH_EINVAL */
#define TH_ENCCTL_SET_DUP_COUNT (18)               /* buf = int: the next N packets after the next frame are duplicates;
                                                      N < 1 << keyframe_granule_shift when the shift is not 0, else TH_EINVAL
                                                      (a duplicate's granule counts it in the shift's bits) */
#define TH_ENCCTL_SET_QUALITY (28)                 /* buf = int 0..63: from the next frame on; TH_EINVAL in bitrate mode */
#define TH_ENCCTL_SET_BITRATE (30)                 /* buf = long (or int when buf_sz == sizeof(int)): > 0 enters bitrate mode
                                                      or changes its target, from the next frame on; before th_encode_flushheader
                                                      the info header's NOMBR field carries it (clamped to 2^24 - 1); 0 (leave
                                                      bitrate mode) TH_EIMPL; < 0 TH_EINVAL */
#define TH_ENCCTL_SET_RATE_FLAGS (20)              /* buf = int, TH_RATECTL_*: in bitrate mode (default DROP_FRAMES | CAP_OVERFLOW),
                                                      else TH_EIMPL */
#define TH_ENCCTL_SET_RATE_BUFFER (22)             /* buf = int, frames: clamped to [12, 256] and written back; in bitrate mode,
                                                      else TH_EIMPL */
#define TH_RATECTL_DROP_FRAMES (0x1)
#define TH_RATECTL_CAP_OVERFLOW (0x2)
#define TH_RATECTL_CAP_UNDERFLOW (0x4)
/* buf = th_huff_code[TH_NHUFFMAN_TABLES][TH_NDCT_TOKENS] and buf_sz exactly its size (2560 x sizeof(th_huff_code)): the codes
   replace the context's ("Huffman codes" above).  buf = NULL with buf_sz = 0: the built-in codes again.  Both only before the first
   th_encode_flushheader has returned a packet and before the first frame, else TH_EINVAL.  A code set that is not valid: TH_EINVAL,
   and the context's codes stay as they were.  ANY OTHER buf_sz: TH_EIMPL, where libtheora answers TH_EINVAL -- the one deviation,
   kept because callers probe this request with an int to learn that custom codes were not available.  Never touches the GPU. */
#define TH_ENCCTL_SET_HUFFMAN_CODES (0)
/* The quantisation parameters of a stream, libtheora's types (codec.h) with its layout: sizeof(th_quant_info) is 464.  A base
   matrix is in natural order.  qi_ranges[qti][pli] (qti 0 intra, 1 inter; pli Y, Cb, Cr): nranges ranges of sizes[] qi steps each,
   summing to 63, and the nranges + 1 base matrices at their ends (spec 6.4.2, 6.4.3). */
typedef uint16_t ogg_uint16_t;
typedef unsigned char th_quant_base[64];
typedef struct th_quant_ranges {
  int nranges;
  const int *sizes;
  const th_quant_base *base_matrices;
} th_quant_ranges;
typedef struct th_quant_info {
  ogg_uint16_t dc_scale[64];
  ogg_uint16_t ac_scale[64];
  unsigned char loop_filter_limits[64];
  th_quant_ranges qi_ranges[2][3];
} th_quant_info;
/* buf = th_quant_info * and buf_sz exactly sizeof(th_quant_info): the parameters replace the context's ("Quantisation parameters"
   above); the encoder takes a deep copy, the caller's arrays may go away.  buf = NULL with buf_sz = 0: the built-in parameters
   again.  Both only before the first th_encode_flushheader has returned a packet and before the first frame, else TH_EINVAL.  A
   set that is not valid: TH_EINVAL, and the context's parameters stay as they were.  ANY OTHER buf_sz: TH_EIMPL, the deviation
   request 0 keeps, for the same reason.  Never touches the GPU. */
#define TH_ENCCTL_SET_QUANT_PARAMS (2)
/* Known, and answered TH_EIMPL: */
#define TH_ENCCTL_SET_VP3_COMPATIBLE (10)
#define TH_ENCCTL_GET_SPLEVEL (16)
#define TH_ENCCTL_2PASS_OUT (24)                   /* (libtheora's two-pass requests and its record format: not these.  A caller */
#define TH_ENCCTL_2PASS_IN (26)                    /*  ported from libtheora uses TH_ENCCTL_THIP_2PASS_OUT / _IN below instead) */
#define TH_ENCCTL_SET_COMPAT_CONFIG (32)

/* Extension: buf = thip_enc_device_in.  What th_encode_ycbcr_in does, with plane pointers in device memory on the context's GPU
   (TH_ENCCTL_THIP_GET_DEVICE) and of the same sizes (frame or picture).  `stream` is a hipStream_t (NULL: the null stream): the
   encoder reads the planes only after the work queued on that stream so far, and the work queued on it afterwards runs only after
   the encoder has read them -- so the caller may write the buffers again from that stream at once (thip_picture_out's
   ordering, in the other direction).  The call does not wait on the host (in bitrate mode it waits for the rate probe, with automatic
   key frames on for a measured frame's 32 bytes). */
#define TH_ENCCTL_THIP_YCBCR_IN_DEVICE (0x7201)
typedef struct thip_enc_device_in {
  th_img_plane planes[3];
  void *stream;
} thip_enc_device_in;
/* Extension: buf = int, receives the context's device index. */
#define TH_ENCCTL_THIP_GET_DEVICE (0x7202)
/* Extension: buf = thip_enc_frame_stats, describing the last packet th_encode_packetout returned. */
#define TH_ENCCTL_THIP_GET_FRAME_STATS (0x7203)
typedef struct thip_enc_frame_stats {
  int64_t tokens;          /* tokens in stream order, every block's EOB on its own */
  int64_t tokens_merged;   /* after the EOB runs are merged: what the packet holds */
  int64_t bytes;           /* packet bytes (0 for a duplicate) */
  int32_t huff[4];         /* table indices: DC luma, DC chroma, AC luma, AC chroma */
  int32_t overflow;        /* coefficients no value token can carry (0 with valid tables) */
  int32_t qi;
} thip_enc_frame_stats;

/* Extension: buf = double[2], receives for the last frame packet the device stage in milliseconds (HIP events around its work,
   the launches' gaps included) and the host's part of th_encode_packetout (EOB runs, tables, bits). */
#define TH_ENCCTL_THIP_GET_TIMES (0x7204)

/* Extension: buf = int 0 / 1, before the first frame only (else TH_EINVAL): inter frames ("Inter frames" above).  Off by default.
   While on, TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE is honoured as libtheoraenc honours it: the interval is clamped to
   [1, 1 << keyframe_granule_shift] and written back (default 1 << keyframe_granule_shift; with shift 0 every frame is a key frame). */
#define TH_ENCCTL_THIP_SET_INTER_FRAMES (0x7205)
/* Extension: buf = thip_enc_inter_stats, describing the last packet th_encode_packetout returned (with inter frames off too). */
#define TH_ENCCTL_THIP_GET_INTER_STATS (0x7206)
typedef struct thip_enc_inter_stats {
  int32_t key;           /* 1 key frame, 0 inter frame or duplicate */
  int32_t modes[5];      /* macro blocks per mode as the decoder sees them: INTER_NOMV, INTRA, INTER_MV, INTER_MV_LAST,
                            INTER_MV_LAST2 (a key frame: all INTRA; a duplicate or a frame with no coded block: all 0) */
  int32_t coded[3];      /* coded blocks per plane */
  int32_t mode_scheme;   /* 0..7, or -1 when none was written */
  int32_t mv_scheme;     /* 0 VLC, 1 six bits, or -1 when none was written */
} thip_enc_inter_stats;
/* Extension: buf = th_ycbcr_buffer of host planes of the FRAME's size, rows top first: receives the encoder's reconstruction of the
   last frame -- the next frame's reference.  Waits for the device.  TH_EINVAL with inter frames off or before the first packet. */
#define TH_ENCCTL_THIP_GET_RECON (0x7207)

/* Extension: buf = int 0 / 1, before the first frame only (else TH_EINVAL; the call never touches the GPU): all eight macro-block
   modes in inter frames ("All eight modes" above).  Off by default; no effect with inter frames off. */
#define TH_ENCCTL_THIP_SET_INTER_MODES (0x7209)
/* Extension: buf = thip_enc_mode_stats, describing the last packet th_encode_packetout returned (with the modes off too). */
#define TH_ENCCTL_THIP_GET_MODE_STATS (0x720A)
typedef struct thip_enc_mode_stats {
  int32_t modes[8];      /* macro blocks per mode, the spec's numbering: INTER_NOMV, INTRA, INTER_MV, INTER_MV_LAST, INTER_MV_LAST2,
                            GOLDEN_NOMV, GOLDEN_MV, INTER_MV_FOUR (counted as thip_enc_inter_stats counts its five) */
  int32_t vectors;       /* motion vectors written to the packet */
} thip_enc_mode_stats;

/* Extension: buf = int D: 0 off (the default: every packet as without the call), 1..31 block-level qi with that delta ("Block-level
   qi" above); any other value TH_EINVAL.  Before the first frame only (else TH_EINVAL); the call never touches the GPU. */
#define TH_ENCCTL_THIP_SET_BLOCK_QI (0x720B)
/* Extension: buf = thip_enc_block_qi_stats, describing the last packet th_encode_packetout returned (with block qi off too: nqis 1;
   a zero-byte packet: all 0). */
#define TH_ENCCTL_THIP_GET_BLOCK_QI_STATS (0x720C)
typedef struct thip_enc_block_qi_stats {
  int32_t nqis;            /* qi values in the frame header */
  int32_t qis[3];          /* the list (unused entries 0) */
  int32_t blocks[3][3];    /* coded blocks by qii (row) and plane (column) */
  int32_t flag_bits;       /* bits the qii flags took */
} thip_enc_block_qi_stats;

/* Extension: buf = int 0 / 1, from the next frame on: the device packetiser ("Device packetiser" above).  Any other value, and a
   call between th_encode_ycbcr_in and th_encode_packetout, TH_EINVAL.  The call never touches the GPU (the packetiser's buffers are
   made at the first frame that uses it).  Initially what option "enc_device_pack" says (theora_hip.h; default 0). */
#define TH_ENCCTL_THIP_SET_DEVICE_PACK (0x720D)
/* Extension: buf = thip_enc_pack_stats, describing the last packet th_encode_packetout returned (a zero-byte packet: all 0 but
   fallbacks). */
#define TH_ENCCTL_THIP_GET_PACK_STATS (0x720E)
typedef struct thip_enc_pack_stats {
  int32_t device;          /* 1: the token bits were packed on the GPU; 0: by the host (the fall-back included) */
  int32_t phase;           /* header_bits mod 8: the bit of the device's first byte at which the token bits start */
  int64_t header_bits;     /* the host-written bits in front of the tokens: frame header, coded flags, modes, vectors, qii flags */
  int64_t token_bits;      /* the four table indices (16 bits) and the merged tokens; header_bits + token_bits, rounded up to a
                              byte, is the packet */
  double pack_ms;          /* the packetiser's device time: HIP events around its launches and its read-backs (0 on the host) */
  int32_t fallbacks;       /* frames of this context whose bits exceeded the device buffer and were packed by the host */
  int32_t reserved;
} thip_enc_pack_stats;
/* Extension: buf = int t: 0 off (the default: every packet as without the call), 1..4096 automatic key frames with the ratio t / 256
   ("Automatic key frames" above; recommended 230); any other value TH_EINVAL.  Before the first frame only (else TH_EINVAL); the
   call never touches the GPU.  Accepted with inter frames off, where it has no effect. */
#define TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES (0x720F)
/* Extension: buf = thip_enc_cut_stats, describing the last packet th_encode_packetout returned (with the switch off too).  For a frame
   that was not measured -- a key frame by the interval rule, a duplicate, any frame with the switch off -- every field is 0 except
   ratio. */
#define TH_ENCCTL_THIP_GET_CUT_STATS (0x7210)
typedef struct thip_enc_cut_stats {
  int32_t measured;   /* 1: the frame was measured */
  int32_t cut;        /* 1: the measurement made it a key frame */
  int32_t intra_mbs;  /* N */
  int32_t ratio;      /* t in force (0: off) */
  int64_t pred;       /* P */
  int64_t intra;      /* I */
  double measure_ms;  /* HIP events, from the search's launch to the 32 bytes on the host */
} thip_enc_cut_stats;
/* Extension: buf = thip_enc_rate_stats, describing the last packet th_encode_packetout returned; TH_EINVAL outside bitrate mode. */
#define TH_ENCCTL_THIP_GET_RATE_STATS (0x7208)
typedef struct thip_enc_rate_stats {
  int32_t qi;              /* the qi chosen (a dropped frame or a duplicate: the last frame's) */
  int32_t dropped;         /* 1: the controller dropped the frame (a zero-byte packet) */
  int32_t key;             /* 1: coded as a key frame */
  int32_t duplicate;       /* 1: a TH_ENCCTL_SET_DUP_COUNT duplicate (nothing probed; the probe fields are 0) */
  int64_t target;          /* T, bits a frame */
  int64_t fullness_before; /* F before the packet ... */
  int64_t fullness_after;  /* ... and after it */
  int64_t spend;           /* S */
  int64_t estimate;        /* Cur(qi) */
  int64_t actual;          /* A, the packet's bits */
  int64_t probe[64];       /* E[q] as the device measured it */
  int64_t corr[2];         /* c_key, c_inter (Q16) after the packet */
  double probe_ms;         /* the probe's device time (HIP events, from its first launch to its 512 bytes on the host) */
  double control_ms;       /* the host controller's time */
} thip_enc_rate_stats;

/* Extension: buf = thip_enc_rgb_in.  What th_encode_ycbcr_in does, for a picture given as R'G'B' ("R'G'B' input" above); width and
   height must be the context's pic_width and pic_height.  TH_EINVAL in the states where th_encode_ycbcr_in returns it (after the
   last packet, with a frame pending, with duplicates left), for a wrong size, format or `device` value and for a pitch smaller than
   the row; TH_EFAULT for NULL pointers (buf, or a src the format uses); every check comes before the device is touched.
   device = 1: src is device memory on the context's GPU (TH_ENCCTL_THIP_GET_DEVICE), `stream` a hipStream_t (NULL: the null
   stream), ordered like TH_ENCCTL_THIP_YCBCR_IN_DEVICE: the encoder reads the source only after the work queued on that stream so
   far, and the work queued on it afterwards waits only until the conversion has read the source, not for the frame's block
   kernels -- the caller may overwrite its picture at once.  The call does not wait on the host (beyond the waits named above for
   bitrate mode and for measured frames).
   device = 0: src is host memory; the rows are copied into a pinned staging buffer made at first use (free again under the rule
   th_encode_ycbcr_in relies on: the previous packet is out), uploaded with one asynchronous copy and converted on the encoder's
   stream; `stream` is ignored. */
#define TH_ENCCTL_THIP_RGB_IN (0x7211)
typedef struct thip_enc_rgb_in {
  int32_t format;          /* THIP_PIC_RGB24 / _RGBA32 / _RGB_PLANAR (theora_hip.h) */
  int32_t device;          /* 0: src is host memory; 1: device memory on the context's GPU (TH_ENCCTL_THIP_GET_DEVICE) */
  int32_t width, height;   /* must be pic_width, pic_height */
  const void *src[3];      /* [0] only for the interleaved formats */
  int64_t pitch[3];        /* bytes a row */
  void *stream;            /* device = 1: a hipStream_t, as in thip_enc_device_in; ignored for device = 0 */
} thip_enc_rgb_in;

/* Extension: buf = int.  0 (the default): off; THIP_CMP_SSE or THIP_CMP_SSE | THIP_CMP_SSIM (theora_hip.h): on, with those metrics
   ("Quality statistics" above).  Before the first frame only, else TH_EINVAL; TH_EINVAL for any other value.  Never touches the GPU. */
#define TH_ENCCTL_THIP_SET_QUALITY_STATS (0x7212)
/* Extension: buf = thip_enc_quality_stats, describing the last packet th_encode_packetout returned.  Waits for the device (the
   compare was queued by th_encode_packetout).  With the switch off, and before the first packet, everything is 0. */
#define TH_ENCCTL_THIP_GET_QUALITY_STATS (0x7213)
typedef struct thip_enc_quality_stats {
  int32_t measured;        /* 1: the packet's picture was compared with its source; 0: a duplicate, or the switch is off */
  int32_t flags;           /* the metrics made: THIP_CMP_* */
  int64_t sse[3];          /* thip_picture_metrics' fields over th_info's picture region ... */
  int64_t samples[3];
  int64_t ssim_q20[3];
  int64_t windows[3];
  double compare_ms;       /* the compare's device time (HIP events around it on the encoder's stream) */
} thip_enc_quality_stats;

/* Extension: buf = int k: 0 off (the default: every packet as without the call), 2..16 activity masking with that ratio ("Activity
   masking" above; recommended 4, libtheora's); any other value TH_EINVAL.  Before the first frame only (else TH_EINVAL); the call
   never touches the GPU.  Accepted with block qi off, where it has no effect. */
#define TH_ENCCTL_THIP_SET_MASKING (0x7214)
/* Extension: buf = thip_enc_mask_stats, describing the last packet th_encode_packetout returned (with the switch off too).  For a
   frame coded without masking -- a duplicate, a dropped frame, a zero-byte packet, any frame with block qi or the switch off --
   every field is 0 except ratio. */
#define TH_ENCCTL_THIP_GET_MASK_STATS (0x7215)
typedef struct thip_enc_mask_stats {
  int32_t ratio;          /* k in force (0: off) */
  int32_t measured;       /* 1: the frame's block-qi choice used the scales */
  int64_t activity_avg;   /* A */
  int64_t activity_max;   /* the largest activity of a luma fragment */
  double mask_ms;         /* HIP events around the two launches */
} thip_enc_mask_stats;

/* Extension: buf = int 0 / 1: the macro-block modes of eight-mode inter frames by the least D + lambda R ("Rate-distortion mode
   decision" above); any other value TH_EINVAL.  Off by default: every packet as without the call.  Before the first frame only (else
   TH_EINVAL); the call never touches the GPU.  Accepted with inter frames or all eight modes off, where it has no effect.
   (0x7216 and 0x7217 are not used.) */
#define TH_ENCCTL_THIP_SET_RD_MODES (0x7218)
/* Extension: buf = thip_enc_rd_stats, describing the last packet th_encode_packetout returned (with the switch off too).  For a frame
   not decided this way -- a key frame, a duplicate, a dropped frame, a zero-byte packet, any frame with five modes or the switch off
   -- every field is 0 except on. */
#define TH_ENCCTL_THIP_GET_RD_STATS (0x7219)
typedef struct thip_enc_rd_stats {
  int32_t on;             /* the switch */
  int32_t measured;       /* 1: the frame's macro-block modes were chosen by the rule */
  int32_t huff[4];        /* the tables the rule counted with: DC luma, DC chroma, AC luma, AC chroma */
  int64_t lambda;         /* the rule's lambda */
  double rd_ms;           /* HIP events around the two launches */
} thip_enc_rd_stats;

/* Extension: buf = int 0 / 1: coded blocks of inter frames are left uncoded where that costs less ("Skip decision" above); any other
   value TH_EINVAL.  Off by default: every packet as without the call.  Before the first frame only (else TH_EINVAL); the call never
   touches the GPU.  Accepted with inter frames off, where it has no effect. */
#define TH_ENCCTL_THIP_SET_RD_SKIP (0x721E)
/* Extension: buf = thip_enc_skip_stats, describing the last packet th_encode_packetout returned (with the switch off too).  For a
   frame not decided this way -- a key frame, a duplicate, a dropped frame, a zero-byte packet, any frame with the switch off -- every
   field is 0 except on. */
#define TH_ENCCTL_THIP_GET_SKIP_STATS (0x721F)
typedef struct thip_enc_skip_stats {   /* 40 bytes */
  int32_t on;             /* the switch */
  int32_t measured;       /* 1: the frame's coded blocks went through the test */
  int32_t skipped[3];     /* per plane: the blocks the test left uncoded (blocks uncoded by the rules before it are not counted) */
  int32_t demoted;        /* macro blocks that lost their mode: no luma block coded, and the test left at least one of the four out */
  int64_t lambda;         /* the frame's unscaled lambda: (s1 * s1 * 40) >> 7, s1 the inter luma step at zig-zag index 1 of qis[0] */
  double skip_ms;         /* HIP events around the two launches */
} thip_enc_skip_stats;

/* Extension: buf = int w: 0 off (the default: every packet as without the call), 1..64 the AC levels of coded blocks are chosen by the
   least D + lambda R with lambda's weight w / 16 ("Level choice" above); any other value TH_EINVAL.  Before the first frame only (else
   TH_EINVAL); the call never touches the GPU.  Recommended: 3 (DESIGN.md section 5.19 has the measurements). */
#define TH_ENCCTL_THIP_SET_RD_QUANT (0x7222)
/* Extension: buf = thip_enc_rd_quant_stats, describing the last packet th_encode_packetout returned (with the switch off too).  For a
   frame not treated -- a duplicate, a dropped frame, a zero-byte packet, any frame with the switch off -- every field is 0 except
   weight.  (0x7220 and 0x7221 are not used: unknown requests, TH_EIMPL.) */
#define TH_ENCCTL_THIP_GET_RD_QUANT_STATS (0x7223)
typedef struct thip_enc_rd_quant_stats {   /* 88 bytes */
  int32_t weight;         /* the switch: w */
  int32_t measured;       /* 1: the frame's coded blocks went through the choice */
  int32_t zeroed[3];      /* per plane: levels +-1 that became 0 */
  int32_t lowered[3];     /* per plane: levels with |l| >= 2 that became l - sgn(l) */
  int32_t emptied;        /* coded blocks that had a non-zero AC level and were left with none */
  int32_t reserved;
  int64_t rate_before;    /* the sums over the coded blocks of R(l) and R(l'), */
  int64_t rate_after;
  int64_t dist_before;    /* ... and of sum over z >= 1 of (c_z - l_z s_z)^2 with l and with l' */
  int64_t dist_after;
  int64_t lambda;         /* the frame's unscaled lambda: (s1 * s1 * 40) >> 7, s1 the luma step at zig-zag index 1 of qis[0] in the
                             frame's own tables (intra on a key frame, inter on an inter frame) */
  double rdq_ms;          /* HIP events around the launch */
} thip_enc_rd_quant_stats;

/* Extension: buf = thip_enc_roi_map: the importance map of "Region of interest" above, for every frame submitted after the call until
   it is replaced; map == NULL clears it (the other fields are then ignored).  Allowed before and between frames -- a map follows the
   content --, but TH_EINVAL with a frame pending and after the last packet.  The encoder takes its own copy at the call:
   device = 0: map is host memory; every entry is checked (one outside -64..64: TH_EINVAL, and the map in force stays) and the rows
   are copied before the call returns; `stream` is ignored.
   device = 1: map is device memory on the context's GPU (TH_ENCCTL_THIP_GET_DEVICE), `stream` a hipStream_t (NULL: the null stream),
   ordered as TH_ENCCTL_THIP_RGB_IN orders its source: the copy reads the map only after the work queued on that stream so far, and
   work queued on it afterwards waits for the copy alone, so the caller may overwrite its tensor from that stream at once.  The
   entries are checked on the device, which cannot refuse: unlike a host map's, an entry outside -64..64 is clamped to +-64 and
   counted (thip_enc_roi_stats.clamped).  The call does not wait on the host.
   TH_EFAULT: enc or buf NULL.  TH_EINVAL: a wrong buf_sz, width or height outside 1..16384, |pitch| < width, device not 0 or 1, a
   host entry out of range -- all found before a device is touched.  Accepted with block qi off, where it has no effect.
   Set the switches first: a TH_ENCCTL_THIP_SET_INTER_FRAMES that changes the switch rebuilds the device state, and the map goes with it.
   (0x7224 is not used: an unknown request, TH_EIMPL.) */
#define TH_ENCCTL_THIP_SET_ROI_MAP (0x7225)
typedef struct thip_enc_roi_map {   /* 40 bytes */
  int32_t width, height;   /* Wm, Hm */
  int32_t device;          /* 0: map is host memory; 1: device memory on the context's GPU */
  int32_t pad;
  int64_t pitch;           /* bytes from one row to the next one down; it may be negative */
  const int8_t *map;       /* row 0 (the picture's top row), or NULL: no map */
  void *stream;            /* device = 1: a hipStream_t, as in thip_enc_rgb_in; ignored for device = 0 */
} thip_enc_roi_map;
/* Extension: buf = thip_enc_roi_stats, describing the last packet th_encode_packetout returned.  For a frame coded without a map -- a
   duplicate, a dropped frame, a zero-byte packet, any frame with block qi off or no map set -- every field is 0 except active,
   map_width and map_height. */
#define TH_ENCCTL_THIP_GET_ROI_STATS (0x7226)
typedef struct thip_enc_roi_stats {   /* 56 bytes */
  int32_t active;          /* 1: a map is set */
  int32_t measured;        /* 1: the frame's block-qi choice used it */
  int32_t map_width, map_height;   /* of the map in force */
  int32_t exp_min, exp_max;        /* the least and greatest exponent e of a luma fragment */
  int64_t exp_sum;                 /* ... and their sum */
  int32_t scale_min, scale_max;    /* the least and greatest final scale i_b of a fragment of any plane */
  int32_t clamped;         /* entries of the frame's map that the device copy clamped (a host map: 0) */
  int32_t reserved;
  double roi_ms;           /* HIP events around the two launches */
} thip_enc_roi_stats;

/* Extension: buf = thip_enc_token_hist, describing the last packet th_encode_packetout returned ("Huffman codes" above).  A
   zero-byte packet, a duplicate and a dropped frame give all zeros.  With the device packetiser the counts come back with the
   record the packet waits for anyway (1 280 more bytes in the same copy); the request itself never touches the GPU. */
#define TH_ENCCTL_THIP_GET_TOKEN_HIST (0x7227)
typedef struct thip_enc_token_hist {   /* 1304 bytes */
  uint32_t count[5][2][32];  /* merged tokens of the last packet: Huffman group, luma / chroma, token (EOB runs after the merge) */
  int32_t huff[4];           /* the tables the packet used: DC luma, DC chroma, AC luma, AC chroma */
  int32_t key;               /* 1 key frame, 0 inter */
  int32_t device;            /* 1: counted by the device packetiser */
} thip_enc_token_hist;
/* Extension: buf = th_huff_code[TH_NHUFFMAN_TABLES][TH_NDCT_TOKENS] (buf_sz its size, else TH_EINVAL), receives the codes in force
   (patterns masked to nbits), at any time.  Never touches the GPU. */
#define TH_ENCCTL_THIP_GET_HUFFMAN_CODES (0x7228)

/* Extension: buf = th_quant_info (buf_sz its size, else TH_EINVAL), receives the quantisation parameters in force, at any time:
   the built-in ones, or the deep copy of what TH_ENCCTL_SET_QUANT_PARAMS was given.  The pointers point into the context and stay
   valid until the next TH_ENCCTL_SET_QUANT_PARAMS or th_encode_free.  Never touches the GPU. */
#define TH_ENCCTL_THIP_GET_QUANT_PARAMS (0x7229)
/* The quantisation parameters of any Theora setup header packet (the decoder's own parser reads it), for
   TH_ENCCTL_SET_QUANT_PARAMS: a transcoder keeps its source's quantisers with it.  `out` owns its arrays until
   thip_quant_info_free (which zeroes it; a zeroed or NULL argument is fine).  Each (qti, pli) gets arrays of its own.  Host only, no
   context.  0, or THIP_EFAULT for a NULL argument, TH_EFAULT without memory, and TH_ENOTFORMAT / TH_EBADHEADER as th_decode_headerin
   answers for the same bytes given as the third header (a packet that is no setup header: TH_EBADHEADER). */
int thip_quant_info_from_setup(const unsigned char *packet, size_t bytes, th_quant_info *out);
void thip_quant_info_free(th_quant_info *qi);

/* The trainer of "Huffman codes" above: out = codes trained on the n histograms, from `start` (NULL: the built-in codes).  Host
   arithmetic only, deterministic, no context and no GPU.  rounds 1..64.  stats may be NULL.  hists may be NULL when n = 0 (out =
   start).  Returns 0; THIP_EFAULT (-1) for out NULL or hists NULL with n > 0; THIP_EINVAL (-10) for n > 2^20, rounds out of range
   or a `start` that is not valid.  out may not overlap start. */
typedef struct thip_huff_train_stats {   /* 32 bytes */
  uint64_t bits_start;       /* the total cost under start */
  uint64_t bits_end;         /* ... and under out: <= bits_start */
  int32_t rounds;            /* rounds accepted */
  int32_t dc_tables;         /* DC tables with at least one sample under out */
  int32_t ac_tables;         /* AC tables with at least one sample under out */
  int32_t samples;           /* samples kept, DC and AC together */
} thip_huff_train_stats;
int thip_huff_train(const thip_enc_token_hist *hists, size_t n, const th_huff_code start[TH_NHUFFMAN_TABLES][TH_NDCT_TOKENS], int rounds,
                    th_huff_code out[TH_NHUFFMAN_TABLES][TH_NDCT_TOKENS], thip_huff_train_stats *stats);

/* Extension: the first pass of "Two-pass" above, with TH_ENCCTL_2PASS_OUT's calling convention: buf = unsigned char **, buf_sz ==
   sizeof(unsigned char *) (else TH_EINVAL).  The first call must come before the first frame (else TH_EINVAL; TH_EINVAL too on a
   context that has had TH_ENCCTL_THIP_2PASS_IN); it enters pass 1, in quality or in bitrate mode, and returns the length of the header
   placeholder, *buf pointing at it.  After each th_encode_packetout one call returns that packet's record (264) and a second call 0;
   after the record of the packet that ended the stream (last != 0) the next call returns the finished header (1084), which the
   caller writes over the placeholder at offset 0.  *buf points at memory of the context, valid until the next call on it.  The call
   never touches the GPU.  (Requests 24 and 26, libtheora's numbers, keep answering TH_EIMPL: the records are not libtheora's.
   0x721A is not used, like 0x7216 and 0x7217: it stays an unknown request, TH_EIMPL whatever the buffer.) */
#define TH_ENCCTL_THIP_2PASS_OUT (0x721D)
/* Extension: the second pass, with TH_ENCCTL_2PASS_IN's calling convention: buf = the pass file's bytes, buf_sz their count; returns
   the number of bytes consumed (all of them, until every record the header counts is in: further bytes are not consumed).  The bytes may
   come in any chunking and ahead of time.  buf == NULL: returns how many more bytes the encoder wants before it can take the next
   frame (0: none).  The first call must come before the first frame and in bitrate mode, on a context not in pass 1, else TH_EINVAL;
   set the other switches (inter frames among them) first.  TH_ENOTFORMAT for a bad magic or version, TH_EINVAL for a header whose
   geometry, fps, key-frame shift or inter-frame switch is not the context's; either leaves the context as it was before the pass file's
   first byte.  While frame n's record has not arrived, and for n >= frames + duplicates of the header, th_encode_ycbcr_in,
   TH_ENCCTL_THIP_YCBCR_IN_DEVICE and TH_ENCCTL_THIP_RGB_IN return TH_EINVAL (before the device is touched).  Never touches the GPU. */
#define TH_ENCCTL_THIP_2PASS_IN (0x721B)
/* Extension: buf = thip_enc_2pass_stats, describing the last packet th_encode_packetout returned (all 0 but pass before the first). */
#define TH_ENCCTL_THIP_GET_2PASS_STATS (0x721C)
#define THIP_2PASS_HEADER_BYTES (1084)
#define THIP_2PASS_RECORD_BYTES (264)
typedef struct thip_enc_2pass_stats {
  int32_t pass;            /* 0: neither; 1: TH_ENCCTL_THIP_2PASS_OUT; 2: TH_ENCCTL_THIP_2PASS_IN */
  int32_t type;            /* pass 1: the record's type (0 key, 1 inter, 2 duplicate, 3 dropped); pass 2: the type of the record the
                              frame followed (a duplicate packet: 2); pass 0: 0 */
  int64_t frame;           /* the packet's index, counted from 0 with the duplicates */
  int32_t qi;              /* the frame's qis[0] */
  int32_t reserved;
  int64_t recorded[64];    /* pass 1: E[q] as written to the record; pass 2: the record's E[q] */
  int64_t fresh[64];       /* the probe of this pass (a duplicate: 0) */
  int64_t budget_left;     /* pass 2: B - A after the packet */
  int64_t recorded_left;   /* pass 2: the sum over the classes of Tot[qi] - Seen[qi] after the frame's record was added */
  int64_t corr[4];         /* pass 2: c_key, c_inter after the packet, and Fresh[u][qi] / Seen[u][qi] in Q16 for u = 0, 1 as the
                              choice saw them (65536 where Seen is 0) */
  double wait_ms;          /* pass 1 in quality mode: the host's wait in th_encode_packetout for the probe's 512 bytes */
  double probe_ms;         /* the probe's device time in this pass (HIP events, from its first launch to its 512 bytes on the host);
                              in bitrate mode thip_enc_rate_stats.probe_ms */
} thip_enc_2pass_stats;

typedef struct th_enc_ctx th_enc_ctx;

/* theoraenc.h:456-537 */
th_enc_ctx *th_encode_alloc(const th_info *info);
/* Extension: the same with the GPU chosen, as th_decode_alloc_on: device 0 .. thip_device_count()-1, or -1 for what
   th_encode_alloc does (option "device", else the calling thread's current device at the first frame). */
th_enc_ctx *th_encode_alloc_on(const th_info *info, int device);
int th_encode_ctl(th_enc_ctx *enc, int req, void *buf, size_t buf_sz);
int th_encode_flushheader(th_enc_ctx *enc, th_comment *comments, ogg_packet *op);
int th_encode_ycbcr_in(th_enc_ctx *enc, th_ycbcr_buffer ycbcr);
int th_encode_packetout(th_enc_ctx *enc, int last, ogg_packet *op);
void th_encode_free(th_enc_ctx *enc);

#ifdef __cplusplus
}
#endif
#endif
