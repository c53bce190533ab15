/* sfnative_effnet.h — weight structs of the EfficientNet trunk entry points of sfnative.h (sf_effnet_trunk_fwd, sf_mbconv_fwd and the
 * single launches).  An extension header: the public struct set of sfnative.h and its SF_ABI_VERSION do not change with it.  The structs
 * here are guarded by SF_EFFNET_ABI_VERSION, which changes whenever one of them changes layout; hosts zero-initialise them. */
#ifndef SFNATIVE_EFFNET_H
#define SFNATIVE_EFFNET_H
#include "sfnative.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MBConv block of the EfficientNet trunk (efficientnet_pytorch model.py MBConvBlock, eval mode), see sf_effnet_trunk_fwd.  The two 1x1
 * layers are sf_conv_w packs with the BatchNorm fold in scale / bias; their `act` is not read: expand is followed by swish, project by none. */
typedef struct sf_mbconv_w {
  sf_conv_w expand;  /* _expand_conv + _bn0; w == NULL at expand ratio 1 (then cexp == cin) */
  sf_conv_w project; /* _project_conv + _bn2, cin = cexp */
  const float *dw_w /*[k*k][cexp]*/, *dw_scale, *dw_bias;   /* _depthwise_conv + _bn1 fold */
  const float *se_reduce_w /*[cse][cexp]*/, *se_reduce_b, *se_expand_w /*[cexp][cse]*/, *se_expand_b;
  int32_t cin, cexp, cout, cse, k, stride;
  int32_t pad_t, pad_l, pad_b, pad_r; /* zero padding of the depthwise layer: top, left, bottom, right */
  int32_t skip;                       /* 1: the block's input is added to its output (stride 1 and cin == cout only) */
  int32_t reserved;
} sf_mbconv_w;

/* EfficientNet trunk as streamingflow/models/encoder.py walks it: stem + n_blocks MBConv blocks (the blocks behind the break index do not exist) */
typedef struct sf_effnet_w {
  const float *stem_w /*[27][c_stem], row (ky*3 + kx)*3 + c*/, *stem_scale, *stem_bias; /* _conv_stem (3x3, stride 2) + _bn0 fold */
  const sf_mbconv_w* blocks; /* HOST array of n_blocks */
  int32_t c_stem, n_blocks;
  int32_t pad_t, pad_l, pad_b, pad_r; /* zero padding of the stem */
  int32_t index;                      /* log2(DOWNSAMPLE): the outputs are reduction_{index + 1} and reduction_{index} */
  int32_t reserved;
} sf_effnet_w;

/* SF_OK when this header's version and struct sizes are the library's, SF_ERR_INVALID otherwise: call once after loading */
static inline int sf_effnet_abi_check_header(void) {
  return sf_effnet_abi_version() == SF_EFFNET_ABI_VERSION && sf_effnet_abi_sizeof(SF_EFFNET_STRUCT_MBCONV_W) == sizeof(sf_mbconv_w) &&
                 sf_effnet_abi_sizeof(SF_EFFNET_STRUCT_EFFNET_W) == sizeof(sf_effnet_w)
             ? SF_OK
             : SF_ERR_INVALID;
}

#ifdef __cplusplus
}
#endif
#endif /* SFNATIVE_EFFNET_H */
