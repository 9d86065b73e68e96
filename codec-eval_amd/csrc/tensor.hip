// Tensor ingest on the device (include/ce_metrics.h: ce_batch_set_*_tensor, ce_tensor_to_*): a
// framework's strided image tensors - u8 / u16 / f16 / bf16 / f32, planar, interleaved, pitched, gray - into the packed RGB
// slots of a resident batch, all images of a call in one launch.  The per-sample rule (clamp, one f32 multiply, rint or
// floor; a linear slot: the clamp of a linear image) is stated in the header.
//
// A streaming kernel of 3 to 12 bytes per pixel in and 3 to 12 out, shaped like k_alpha: a thread owns the pixels of 48
// output bytes of one row (16 of a u8 slot, 8 of a u16 slot, 4 of an f32 slot), reads them in 16-byte loads where the
// launch's strides and base allow (tensor_ladder.h: tensor_pick_path) and stores its 48 bytes as three 16-byte words where the
// address allows, falling back on its own to 8-, 4-, 2- or 1-byte stores.  Image n is blockIdx.y.  No LDS, no scratch.
#include "ce_internal.h"

#include "tensor_kernel.h"
#include "tensor_ladder.h"

int ce_launch_tensor(ce_ctx *ctx, hipStream_t stream, const ce_tensor_dev &src, uint32_t w, uint32_t h, uint32_t count, void *d_dst,
                     size_t slot_bytes, int slot, uint32_t depth)
{
    if (w == 0 || h == 0 || count == 0) return CE_OK;
    if (slot < TENSOR_SLOT_U8 || slot > TENSOR_SLOT_LIN) {
        ctx->err = "tensor ingest: bad launch";
        return CE_ERR_INVALID_ARG;
    }
    if (w > 0xfffffff0u || count > 65535u) {
        ctx->err = "tensor ingest: image too large or too many images for one launch";
        return CE_ERR_INVALID_ARG;
    }
    const tensor_args a = tensor_make_args(src.dtype, src.quantise, src.data, src.stride_n, src.stride_c, src.stride_y, src.stride_x, w, h, count, d_dst,
                                           slot_bytes, slot, depth);
    const size_t blocks = tensor_blocks(a);
    if (blocks > 0x7fffffffu / kTensorBlock) {
        ctx->err = "tensor ingest: image too large or too many images for one launch";
        return CE_ERR_INVALID_ARG;
    }
    const dim3 grid((uint32_t)blocks, count), block(kTensorBlock);
    const bool known = tensor_ladder(src.dtype, slot, [&](auto dt, auto sl) {
        constexpr int DT = decltype(dt)::value, SLOT = decltype(sl)::value;
        CE_LAUNCH_ON(ctx, stream, tensor_profile_name(DT, SLOT, count > 1).s, (k_tensor<DT, SLOT>), grid, block, 0, a);
    });
    if (!known) {
        ctx->err = "tensor ingest: this dtype does not enter this slot";
        return CE_ERR_INVALID_ARG;
    }
    CE_HIP(ctx, hipGetLastError());
    return CE_OK;
}
