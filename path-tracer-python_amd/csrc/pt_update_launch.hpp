// pt_update_launch.hpp — the host half of the scene-update ABI that the pose
// ABI shares (pt_update.hip defines it, pt_pose.hip calls it): the checks of the
// scene and the topology, and the launches of step 2 (the refit, in both forms)
// and of the root copy. Host only; the kernels themselves stay pt_update.hip's.
#pragma once
#include <stdint.h>

#include "../../include/ptmi_update.h"

namespace ptmi {

// The scene's counts checked; `what` ("update", "pose") begins the message.
int upd_check_scene(const ptmi_scene_view* scene, const char* what);

// ref_nodes, nodes, the topology and root_box checked for a call with n_edits
// edits in all: everything ptmi_update_primitives rejects after its lists.
int upd_check_tree(const ptmi_scene_view* scene, const ptmi_update_topology* topo, const float* root_box,
                   int64_t n_edits, const char* what);

// Step 2 and the root copy of a checked call, on `stream`. No HIP result is read.
void upd_refit_launch(const ptmi_scene_view* scene, const ptmi_update_topology* topo, float* root_box, void* stream);

}  // namespace ptmi
