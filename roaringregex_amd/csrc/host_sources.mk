# The host pipeline - pattern -> automaton -> device programs -> packed images, no HIP in it - named once.  csrc/Makefile and the
# Makefiles under tools/ include this file; tests/program_replay.py (host_pipeline_sources) reads HOST_SRCS from it.
LOWER_SRCS = lower_trim.cpp lower_reduce.cpp lower_nfa.cpp lower_dfa.cpp lower_tables.cpp table_order.cpp
HOST_SRCS = frontend.cpp $(LOWER_SRCS) pack.cpp plan.cpp
HOST_HDRS = frontend.hpp lower.hpp lower_internal.hpp table_order.hpp once_task.hpp pack.hpp plan.hpp device.hpp
# with the sampled table's life (sampled.cpp: host code too)
HOST_SAMPLED_SRCS = $(HOST_SRCS) sampled.cpp
HOST_SAMPLED_HDRS = $(HOST_HDRS) sampled.hpp
