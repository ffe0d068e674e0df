# Builds libbcmpc.so (HIP for gfx950) in-tree.  `make -j` is safe; no cmake.
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-function
SRC      := bc_mpc_amd/csrc
LIB      := bc_mpc_amd/libbcmpc.so
# objects by how they compile: host units that see the kernels' launch headers (hipcc -x hip), plain C++ (g++),
# every other one a kernel unit (.hip); OBJ in link order
HOSTOBJ  := capi cost_terms engine_plan pack mt_draw planners
CXXOBJ   := mt19937 mt_jump ac_fit_plan ac_ppo_plan
OBJ      := $(patsubst %,build/%.o,rollout rollout_grp rollout_x3 rollout_x3_plain rollout_pp rollout_team cem mppi batch \
              plan_batch plan_noise plan_prop plan_knots mppi_ext term_cost terminal_value ensemble fit ac_fit ac_ppo $(HOSTOBJ) $(CXXOBJ) mt_device comm)
# header dependencies come from the compiler (build/*.d): a header rebuilds exactly the objects that include it
DEPFLAGS := -MMD -MP

all: $(LIB)

# the split kernels in three units, each with the scheduler that measured best
# (profiles/r01_sched_ilp_ab.txt, profiles/r01_sched_part2_ab.txt): the plain tanh delta net
# (rollout_x3_plain) with iterative-ILP (-1..2% kernel time at cfg3/cfg4); the policy / reward / relu-LN /
# single-pass kernels (rollout_x3) and the two pipelined kernels (rollout_pp) with max-ILP
# (-0.6..1.7%; iterative-ILP spills the policy+reward kernel, +10%)
X3ILP    ?= -mllvm -amdgpu-sched-strategy=iterative-ilp
X3P2     ?= -mllvm -amdgpu-sched-strategy=max-ilp
build/rollout_x3.o:       EXTRA = $(X3P2)
build/rollout_pp.o:       EXTRA = $(X3P2)
build/rollout_x3_plain.o: EXTRA = $(X3ILP)

# the team kernels with the iterative ILP scheduler: ppo_defaults -2.4 us, ppo_mpc_default -5.5 us, run.sh
# recipe -4.8 us per call against the default (max-ilp +2.5..+21 us, iterative-minreg +0..+24 us;
# profiles/r04_team_sched_ab.jsonl)
TEAMSCHED ?= -mllvm -amdgpu-sched-strategy=iterative-ilp
build/rollout_team.o:     EXTRA = $(TEAMSCHED)

HIPCOMPILE = $(strip $(HIPCC) $(HIPFLAGS) $(EXTRA) $(DEPFLAGS) -c $< -o $@)

build/%.o: $(SRC)/%.hip
	@mkdir -p build
	$(HIPCOMPILE)

$(HOSTOBJ:%=build/%.o): build/%.o: $(SRC)/%.cpp
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -x hip $(DEPFLAGS) -c $< -o $@

$(CXXOBJ:%=build/%.o): build/%.o: $(SRC)/%.cpp
	@mkdir -p build
	g++ -O3 -std=c++17 -fPIC -ffp-contract=off -Wall $(DEPFLAGS) -c $< -o $@

-include $(OBJ:.o=.d)

$(LIB): $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(OBJ) -ldl

# resource usage report (VGPR/SGPR/LDS/occupancy) for the rollout kernels
resources: $(SRC)/rollout.hip $(SRC)/rollout_grp.hip
	$(HIPCC) $(HIPFLAGS) -c $(SRC)/rollout.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs:|AGPRs|Spill|Occupancy|LDS"
	$(HIPCC) $(HIPFLAGS) -c $(SRC)/rollout_grp.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs:|AGPRs|Spill|Occupancy|LDS" 

asm: $(SRC)/rollout.hip $(SRC)/rollout_grp.hip
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -S --cuda-device-only $(SRC)/rollout.hip -o build/rollout.s
	$(HIPCC) $(HIPFLAGS) -S --cuda-device-only $(SRC)/rollout_grp.hip -o build/rollout_grp.s

clean:
	rm -rf build $(LIB)

.PHONY: all clean resources asm
