// Compiled by tests/test_gpu_step_plan.py: walks one default.yaml hexapod through the façade and prints what its LegStepper getters of the
// step plan (getSwing1ControlNode .. getWalkPlaneNormal) return for every leg, one line per getter; the test compares the lines with the columns
// of the step plan pass, which it reads from the same engine in one call and prints as well.
#include "shc_facade.hpp"
#include <cstdio>
#include <cstdlib>

using namespace shc_facade;

static void line(const char *name, int leg, int i, const Vector3 &v) { printf("%s %d %d %.17g %.17g %.17g\n", name, leg, i, v[0], v[1], v[2]); }

int main(int argc, char **argv) {
  if (argc < 6) return 2;
  FILE *f = fopen(argv[1], "rb");
  shc_params p;
  if (!f || fread(&p, sizeof p, 1, f) != 1) return 3;
  fclose(f);
  if ((int64_t)sizeof p != shc_sizeof_params()) return 4;
  const int cycles = atoi(argv[2]);
  double v[2] = {atof(argv[3]), atof(argv[4])};
  const double w = atof(argv[5]);
  auto engine = std::make_shared<Engine>(p, 1, 0);
  auto model = std::make_shared<Model>(engine);
  auto walker = std::make_shared<WalkController>(engine);
  for (int c = 0; c < cycles; ++c) {
    walker->updateWalk(v, w);
    model->updateModel();
  }
  for (int l = 0; l < model->getLegCount(); ++l) {
    const LegStepper stepper = model->getLegByIDNumber(l).getLegStepper();
    for (int i = 0; i < 5; ++i) {
      line("swing_1_nodes", l, i, stepper.getSwing1ControlNode(i));
      line("swing_2_nodes", l, i, stepper.getSwing2ControlNode(i));
      line("stance_nodes", l, i, stepper.getStanceControlNode(i));
    }
    line("stride_vector", l, 0, stepper.getStrideVector());
    line("swing_clearance", l, 0, stepper.getSwingClearance());
    line("default_tip", l, 0, stepper.getDefaultTipPosition());
    line("target_tip", l, 0, stepper.getTargetTipPosition());
    line("walk_plane", l, 0, stepper.getWalkPlane());
    line("walk_plane_normal", l, 0, stepper.getWalkPlaneNormal());
  }
  try {
    model->getLegByIDNumber(0).getLegStepper().getStanceControlNode(5);
    return 5;
  } catch (const std::out_of_range &) {
    printf("node 5 refused\n");
  }
  // the same fields in one call of the pass on the same engine: the row the getters are compared with
  shc_plan_spec spec{};
  const int fields[] = {SHC_PLAN_SWING_1_NODES,  SHC_PLAN_SWING_2_NODES,   SHC_PLAN_STANCE_NODES, SHC_PLAN_DEFAULT_TIP,      SHC_PLAN_TARGET_TIP,
                        SHC_PLAN_STRIDE_VECTOR, SHC_PLAN_SWING_CLEARANCE, SHC_PLAN_WALK_PLANE,   SHC_PLAN_WALK_PLANE_NORMAL};
  spec.n_fields = 9;
  for (int i = 0; i < 9; ++i) spec.fields[i] = fields[i];
  spec.dtype = SHC_OBS_F64, spec.legs = model->getLegCount(), spec.pad = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> row(size_t(shc_plan_width(&spec)));
  if (shc_engine_get_step_plan(engine->handle(), 0, 1, &spec, row.data(), 0) != SHC_OK) return 6;
  printf("row");
  for (double x : row) printf(" %.17g", x);
  printf("\n");
  return 0;
}
