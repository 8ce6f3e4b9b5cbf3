"""Activation-plane layouts (see csrc/mlp_engine.h).

fp32 path: row-major [P, ld].  bf16 path: tile-blocked "PT32": points padded to a multiple of 32; per block and 32-feature
tile [k(2)][h(2)][point(32)][8 features], the 16-byte unit (k, h, point) holding features 16k + 4h + {0..3} and
16k + 8 + 4h + {0..3}: element (p, f) at
(p>>5)*(32*ld) + (f>>5)*1024 + ((f>>4)&1)*512 + ((f>>2)&1)*256 + (p&31)*8 + ((f>>3)&1)*4 + (f&3).
These converters serve the stand-alone module API (SDFNetwork.forward / RenderingNetwork.forward), where
the caller hands over / expects row-major tensors; the render path never converts."""
import torch


def pad32(P):
    return (P + 31) // 32 * 32


def rows(P, precision):
    return P if precision == "fp32" else pad32(P)


def to_pt32(x):
    """[P, ld] float -> bf16 PT32 buffer [pad32(P) * ld]."""
    P, ld = x.shape
    Pp = pad32(P)
    buf = torch.zeros(Pp, ld, dtype=torch.bfloat16, device=x.device)
    buf[:P] = x.to(torch.bfloat16)
    # feature within a tile = 16 k + 8 j + 4 hh + e:  [blk, c, nt, k, j, hh, e] -> [blk, nt, k, hh, c, j, e]
    return buf.view(Pp // 32, 32, ld // 32, 2, 2, 2, 4).permute(0, 2, 3, 5, 1, 4, 6).contiguous().view(-1)


def from_pt32(buf, P, ld):
    """bf16 PT32 buffer -> [P, ld] float32."""
    Pp = pad32(P)
    # [blk, nt, k, hh, c, j, e] -> [blk, c, nt, k, j, hh, e]
    x = buf.view(-1)[:Pp * ld].view(Pp // 32, ld // 32, 2, 2, 32, 2, 4).permute(0, 4, 1, 2, 5, 3, 6).contiguous().view(Pp, ld)
    return x[:P].float()


def decode_chunk_bf16(chunk, kt):
    """One fmt-1 weight chunk (include/vdn_render.h: VdnChunkDesc; uint8 tensor of >= kt * 2048 + 128 bytes) ->
    (W [32, 32 kt] float32, bias [32] float32). The chunk is [kt * 2 k-steps][64 lanes][8 bf16], lane (i, h) = i + 32 h holding
    output row i, element j of k-step s the input k = 16 s + 8 (j >> 2) + 4 h + (j & 3); behind it 32 float32 biases."""
    raw = chunk.reshape(-1)[:kt * 2048 + 128].cpu().contiguous()
    w = raw[:kt * 2048].clone().view(torch.bfloat16).view(2 * kt, 2, 32, 2, 4)           # [s, h, i, j >> 2, j & 3]
    W = w.permute(2, 0, 3, 1, 4).reshape(32, 32 * kt).float()                               # [i, s, j >> 2, h, j & 3]
    return W, raw[kt * 2048:].clone().view(torch.float32)


def decode_chunk_f32(chunk, kt):
    """One fmt-0 weight chunk (csrc/mlp_engine.h, F32; uint8 tensor of >= kt * 4096 + 128 bytes) -> (W [32, 32 kt] float32,
    bias [32] float32). The chunk is [kt * 4 groups][64 lanes][4 f32], lane (i, h) = i + 32 h of group g holding
    W[i][8 g + 4 h .. + 3]; behind it, at byte kt * 4096, 32 float32 biases."""
    raw = chunk.reshape(-1)[:kt * 4096 + 128].cpu().contiguous()
    w = raw[:kt * 4096].clone().view(torch.float32).view(4 * kt, 2, 32, 4)                 # [g, h, i, e]
    return w.permute(2, 0, 1, 3).reshape(32, 32 * kt).contiguous(), raw[kt * 4096:].clone().view(torch.float32)


def col_offset_elems(col0, precision):
    """Element offset of column col0 (a multiple of 32) inside a plane."""
    if precision == "fp32":
        return col0
    assert col0 % 32 == 0
    return (col0 // 32) * 1024


def mask_from_plane(buf, P, ld):
    """1-bit ReLU mask plane of one layer (csrc/mlp_engine.h: BF16::relu_bits) -> bool [P, ld].

    Per block of 32 points: [h(2)][point(32)][ld/16 bytes]; lane (point, h) keeps 16 bits per 32-feature tile, bit 16 tile + t
    (little-endian) = accumulator register t = 8k + 4j + e, feature 32 tile + 16k + 8j + 4h + e (the PT32 order above)."""
    Pp = pad32(P)
    b = buf.reshape(-1)[:Pp * ld // 8].view(Pp // 32, 2, 32, ld // 16).long()
    bits = (b.unsqueeze(-1) >> torch.arange(8, device=b.device)) & 1         # [blk, h, c, byte, bit]: bit 16 tile + t
    bits = bits.reshape(Pp // 32, 2, 32, ld // 32, 2, 2, 4)                   # [blk, h, c, tile, k, j, e]
    return bits.permute(0, 2, 3, 4, 5, 1, 6).reshape(Pp, ld)[:P].bool()     # [blk, c, tile, k, j, h, e]
