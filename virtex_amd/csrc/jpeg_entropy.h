// What the host half (vtx_jpeg_describe in jpeg.hip: markers, tables, segment byte scan) hands to the device Huffman decoder
// (jpeg_entropy.hip): one descriptor per image, all 32-bit words, laid out behind one another in the chunk buffer that crosses
// PCIe together with the scans' bytes.
#pragma once

constexpr int VTX_JPEG_WG = 256;             // lanes per workgroup = subsequences per workgroup; a workgroup serves ONE image
constexpr int VTX_JPEG_MAX_TABLES = 6;       // three components x (DC, AC) at the most

// canonical Huffman decoding table as the host builds it (jpeg.hip, Huff): 9-bit lookahead (symbol << 4 | length, 0 = longer
// code), per length the largest code and the offset of its first symbol.  1 416 bytes.
struct VtxJpegTable {
    unsigned short look[512];
    int maxcode[17];                          // [1..16]; -1 = no code of that length
    int valptr[17];
    unsigned char vals[256];
};

struct VtxJpegSegment { int begin, end, first_sub; };   // scan bytes [begin, end) (relative to the image's bytes), first subsequence

struct VtxJpegDesc {
    int desc_bytes;                           // this struct + Huffman tables + segment table + quantisation tables
    int byte_off, nbytes;                     // the image's scan bytes inside the chunk buffer
    int nsub, nseg, first_wg, nwg;            // subsequences, segments (restart intervals), workgroups [first_wg, first_wg + nwg)
    int subseq_bytes;
    int seg_mcus, total_mcus, mcux, bpm;      // MCUs per segment (all of them without restart intervals), blocks per MCU
    int ncomp, total_blocks;
    int coef_off_lo, coef_off_hi;             // first int16 of the image in the coefficient buffer
    int status_slot;
    int blk_comp[6], blk_h[6], blk_v[6];      // block k of an MCU: its component and position inside the component's MCU patch
    int comp_off[3], comp_bw[3], comp_h[3], comp_v[3];
    int dc_tab[3], ac_tab[3];                 // per component: index into the packed tables
    int ntab, tab_off, seg_off;               // byte offsets from the descriptor's start; nseg + 1 segment entries (a sentinel closes)
    int qt_off;                               // uint16 [4][64] quantisation tables (natural order), for vtx_jpeg_reconstruct
};

// status reasons (second word of an image's status pair; the first is the host decoder's class, VTX_ERR_ARG)
enum { VTX_JPEG_BAD_CODE = 1, VTX_JPEG_BAD_DC = 2, VTX_JPEG_BAD_RUN = 3, VTX_JPEG_BAD_TOTAL = 4 };
