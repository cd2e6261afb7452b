"""The checker for plane input (m1v_set_plane_layout) whose planes are not the image of any RGB picture — TEST INFRASTRUCTURE ONLY.

A Python restatement of the oracle's frame walk (oracle/mpeg1_oracle.c walk_picture / orc_encode_frame, encoder.h:238-458) on the
oracle's own pieces: orc_bits_put for the 38-bit slice header and the 2-bit macroblock header, orc_fdct, orc_quant_zigzag,
orc_encode_block, zero padding per strip; the 44 header bytes are those of orc_encode_frame for a black picture of the same
geometry and frame index, with the length field (bytes 4-5) patched again; four zero bytes close the record.  The samples come
from two callables, so any layout can be fed.  tests/test_planes_abi.py pins it to orc.encode_frame on converted planes.
"""
import ctypes as C

import numpy as np

import oracle_ffi as orc


class Unencodable(ValueError):
    """The oracle's ORC_E_UNENCODABLE: an emitted AC level with |level| >= 256."""
    code = orc.E_UNENCODABLE


def encode_frame(luma_block, chroma_block, W, H, frame_index, qf, mode):
    """One frame record.  luma_block(x, y): the 8x8 bytes whose top-left luma sample is (x, y); chroma_block(p, x, y): the 8x8
    samples of plane p (0 = Cb, 1 = Cr) of the macroblock at (x, y) — uint8 arrays of 64 elements, row-major.  Raises Unencodable
    where the oracle returns ORC_E_UNENCODABLE."""
    L = orc.lib()
    xe, ye = orc.region(mode, W, H)
    assert 0 < xe <= W and 0 < ye <= H
    q = orc.scale_qmatrix(qf)
    qp = q.ctypes.data_as(orc._i32p)
    dct = np.empty(64, np.int32)
    zz = np.empty(64, np.int32)
    dp, zp = dct.ctypes.data_as(orc._i32p), zz.ctypes.data_as(orc._i32p)
    bits = orc.OrcBits()
    L.orc_bits_init(C.byref(bits))
    try:
        def block(px, is_luma):
            blk = np.ascontiguousarray(px, dtype=np.uint8).reshape(64)
            L.orc_fdct(blk.ctypes.data_as(orc._u8p), dp)
            L.orc_quant_zigzag(dp, qp, zp)
            rc = L.orc_encode_block(is_luma, zp, C.byref(bits))
            if rc == orc.E_UNENCODABLE:
                raise Unencodable("plane_oracle: |level| >= 256")
            assert rc == 0, rc

        for x in range(0, xe, 16):
            L.orc_bits_put(C.byref(bits), 0x000001, 24)         # mpeg1_slice, mpeg1_blk.c:12-16
            L.orc_bits_put(C.byref(bits), (x // 16 + 1) & 0xff, 8)
            L.orc_bits_put(C.byref(bits), 1, 5)
            L.orc_bits_put(C.byref(bits), 0, 1)
            for y in range(0, ye, 16):
                L.orc_bits_put(C.byref(bits), 0x3, 2)           # macroblock header, mpeg1_blk.c:38-51
                for b in range(4):
                    block(luma_block(x + (b % 2) * 8, y + (b // 2) * 8), 1)
                for p in range(2):
                    block(chroma_block(p, x, y), 0)
            while bits.nbits & 7:                               # encoder.h:442-443
                L.orc_bits_put(C.byref(bits), 0, 1)
        payload = bytes(bytearray(bits.buf[:bits.nbits >> 3]))
    finally:
        L.orc_bits_free(C.byref(bits))
    head = bytearray(orc.encode_frame(np.zeros((H, W, 3), np.uint8), W, H, frame_index, qf, mode)[:44])
    fwd = (44 + len(payload) - 8) & 0xffff
    head[4], head[5] = fwd >> 8, fwd & 0xff
    return bytes(head) + payload + b"\0\0\0\0"


def layout_samplers(frame, layout):
    """(luma_block, chroma_block) that read one frame's bytes (a flat uint8 array starting at the frame's base) through a plane
    layout: a dict with y_offset, cb_offset, cr_offset, y_pitch, c_pitch, c_step, no zeros — the definition of
    include/mpeg1_hip.h."""
    frame = np.asarray(frame, dtype=np.uint8).reshape(-1)
    rows = np.arange(8)[:, None]
    cols = np.arange(8)[None, :]
    y_off, y_pitch = layout["y_offset"], layout["y_pitch"]
    c_off, c_pitch, c_step = (layout["cb_offset"], layout["cr_offset"]), layout["c_pitch"], layout["c_step"]

    def luma_block(x, y):
        return frame[y_off + (y + rows) * y_pitch + x + cols]

    def chroma_block(p, x, y):
        return frame[c_off[p] + (y // 2 + rows) * c_pitch + (x // 2 + cols) * c_step]

    return luma_block, chroma_block


def encode_layout(frame, layout, W, H, frame_index, qf, mode):
    """encode_frame over layout_samplers(frame, layout)."""
    luma_block, chroma_block = layout_samplers(frame, layout)
    return encode_frame(luma_block, chroma_block, W, H, frame_index, qf, mode)


def reference_layout(W, H):
    """The layout of the planes orc.convert returns, laid Y, Cb, Cr behind one another (the reference's own planes)."""
    return dict(y_offset=0, cb_offset=W * H, cr_offset=2 * W * H, y_pitch=W, c_pitch=W // 2, c_step=1, frame_stride=3 * W * H)
