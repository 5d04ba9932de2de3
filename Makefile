# Convenience targets (the driver uses __graft_entry__.py / bench.py / pytest directly).
PY ?= python

build:            ## hipcc --offload-arch=gfx950 -> adaptive-speculative-decoding_amd/lib/libasd_hip.so, gcc -> oracle
	$(PY) -c "import __graft_entry__ as g; g.build()"

test-cpu:         ## oracle vs goldens, host logic, ABI symbols, gloo 2-rank exchange (no GPU needed)
	$(PY) -m pytest tests -q -m "not gpu"

test-gpu:         ## parity of the HIP path through the C ABI (needs an MI355X)
	$(PY) -m pytest tests -q -m gpu

smoke:
	$(PY) -c "import __graft_entry__ as g; g.smoke()"

bench:
	$(PY) bench.py

golden:           ## regenerate tests/golden from the reference's own files (dev container only)
	PYTHONDONTWRITEBYTECODE=1 $(PY) oracle/gen_golden.py

test-hooks:       ## the TEST build of the library (libasd_hip_test.so: product objects + the asd_debug_* switches under -DASD_TEST_HOOKS)
	$(PY) adaptive-speculative-decoding_amd/build.py --test-hooks

asan-host:        ## host side of the launchers under AddressSanitizer + UBSan (CPU only: the ABI / argument-check tests)
	$(PY) adaptive-speculative-decoding_amd/build.py --asan
	ASD_LIB_PATH=$(CURDIR)/adaptive-speculative-decoding_amd/lib/libasd_hip_asan.so \
	LD_PRELOAD=$$(/opt/rocm/lib/llvm/bin/clang -print-file-name=libclang_rt.asan-x86_64.so) \
	ASAN_OPTIONS=detect_leaks=0:detect_odr_violation=0:verify_asan_link_order=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	$(PY) -m pytest tests/test_abi.py -q -p no:cacheprovider

asan-host-args:   ## stand-alone program (its own main, no Python): the argument checks of asd_residual_sample_lp / asd_commit_step_lp / asd_commit_step_stop / asd_commit_step_finish / asd_verify_greedy / asd_top_logprobs / asd_commit_top_logprobs / asd_step_uniforms / asd_logit_edit_rows / asd_logit_mask_rows / asd_penalty_rows / asd_penalty_commit / asd_bad_words_rows / asd_fsm_mask_rows / asd_fsm_advance / asd_fsm_commit / asd_no_repeat_ngram_rows / asd_prompt_logprobs / asd_token_stats under ASan + UBSan
	$(PY) adaptive-speculative-decoding_amd/build.py --asan
	/opt/rocm/lib/llvm/bin/clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude tools/asan_host_args.cpp \
	  -Ladaptive-speculative-decoding_amd/lib -lasd_hip_asan -L/opt/rocm/lib -lamdhip64 \
	  -Wl,-rpath,$(CURDIR)/adaptive-speculative-decoding_amd/lib -Wl,-rpath,/opt/rocm/lib \
	  -o adaptive-speculative-decoding_amd/lib/asan_host_args
	ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 adaptive-speculative-decoding_amd/lib/asan_host_args

clean:
	rm -rf adaptive-speculative-decoding_amd/lib oracle/_build gpurun_out

.PHONY: build test-cpu test-gpu smoke bench golden test-hooks asan-host asan-host-args clean
