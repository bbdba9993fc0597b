// ABI plumbing shared by every translation unit of libdafne_amd.so.
#include "common.h"

namespace dafne {
char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}
}  // namespace dafne

extern "C" {
int dafne_abi_version(void) { return 155; }  // 0.5.5: dafne_pred_dgrad_gn_hip, dafne_pred_dgrad_gn_workspace_bytes (data gradient of the prediction convolutions through the last GroupNorm of a tower);  // 0.5.4: dafne_pred_wgrad_hip, dafne_pred_wgrad_workspace_bytes (weight / bias gradients of the head's prediction convolutions), dafne_head_uncook_backward_hip, dafne_head_uncook_backward_workspace_bytes (back through the finished regressions, scale gradients);  // 0.5.3: dafne_train_views_u8_hip, dafne_train_gt_hip (augmented training views and their ground truth);  // 0.5.2: dafne_losses_backward_hip, dafne_losses_backward_workspace_bytes (the losses' gradients with respect to the head outputs);  // 0.5.1: dafne_scene_split_labels_hip, dafne_scene_pack_tile_gt_hip (scene labels -> the ground truth of every tile);  // 0.5.0: dafne_bottleneck_body16_hip (the res4 block kernel in the 16x16x32 fragment order, engine.pack_bneck16);  // 0.4.9: dafne_assign_targets_hip, dafne_losses_hip (target assignment and loss values);  // 0.4.8: dafne_scene_scaled_tiles_u8_hip, dafne_scene_merge_rows_scaled_hip, dafne_scene_merge_hbb_rows_scaled_hip (multi-scale whole-scene inference);  // 0.4.7: dafne_hbb_nms_f64_batched_hip, dafne_scene_merge_hbb_rows_hip, dafne_scene_match_hbb_hip (DOTA Task2: horizontal boxes);  // 0.4.6: dafne_bottleneck_block_narrow_s2_hip (the last res2 block at the pixels res3 reads), DAFNE_CONV_RELU_INPUT (dafne_conv2d_wr_hip);  // 0.4.5: dafne_scene_match_hip, dafne_scene_mark_hip (scoring whole scenes against their labels);  // 0.4.4: dafne_scene_views_u8_hip, dafne_tta_candidates_hip (scene-level TTA);  // 0.4.3: dafne_scene_tiles_u8_hip, dafne_scene_merge_rows_hip (whole-scene inference);  // 0.4.2: dafne_decode_params.flags (DAFNE_DECODE_NO_CENTER / _NO_CTRNESS), dafne_corner_chain_hip;  // 0.4.1: DAFNE_CONV_FRAG16 (dafne_conv3x3_c256_hip in the 16x16x32 fragment order);  // 0.4.0: dafne_conv3x3_c256_fp8w_hip removed, dafne_bottleneck_body_hip takes row-permuted weights (engine.pack_bneck);  // 0.3.1: dafne_stem_pool_conv1_hip;  // 0.3.0: dafne_conv2d_wr_*, dafne_bottleneck_block_{narrow,mid}_hip, bottleneck_body without a head, unknown conv flags rejected;  // 0.2.0: per-call NMS flags replace dafne_poly_nms_set_exact_only;  // 0.1.1: dafne_conv_params grew (GN_FINALIZE), b2b weight layout; .1: narrow tail+head
const char* dafne_last_error(void) { return dafne::err_buf(); }
}
