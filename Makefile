# mpix — MI355X-native accelerator-triggered MPI extensions.
# Builds libmpix.so (C API) with hipcc for gfx950. Cross-compiles fine on a
# GPU-less box; the .so loads and runs host-only paths without a GPU.

HIPCC      ?= hipcc
GPU_ARCH   ?= gfx950
MPI_HOME   ?= /opt/conda

CXXFLAGS   := -O3 -std=c++17 -fPIC --offload-arch=$(GPU_ARCH) \
              -Iinclude -I$(MPI_HOME)/include -Wall -Wextra -Wno-unused-parameter
LDFLAGS    := -shared -L$(MPI_HOME)/lib -lmpi -Wl,-rpath,/usr/lib/x86_64-linux-gnu -Wl,-rpath,$(MPI_HOME)/lib

ifdef DEBUG
CXXFLAGS   += -g -DMPIX_DEBUG
endif

SRCS := src/state.cpp src/init.cpp src/proxy.cpp src/enqueue.cpp \
        src/partitioned.cpp src/transport/bootstrap.cpp \
        src/transport/native.cpp src/transport/mpi.cpp
OBJS := $(SRCS:.cpp=.o)

LIB  := libmpix.so
PYEXT := mpix/_C.so
PYINC := $(shell python3 -c "import sysconfig;print(sysconfig.get_paths()['include'])")
PYBIND11INC := $(shell python3 -c "import pybind11;print(pybind11.get_include())")

all: $(LIB) python

python: $(PYEXT)

mpix/_core.o: mpix/_core.cpp include/mpix/mpix.h include/mpix/mpix_device.h \
              include/mpix/mpix_abi.h include/mpix/mpix_layout.h
	$(HIPCC) $(CXXFLAGS) -I$(PYINC) -I$(PYBIND11INC) -c mpix/_core.cpp -o $@

$(PYEXT): mpix/_core.o $(OBJS)
	$(HIPCC) --offload-arch=$(GPU_ARCH) mpix/_core.o $(OBJS) $(LDFLAGS) -o $@

%.o: %.cpp src/internal.h include/mpix/mpix.h include/mpix/mpix_abi.h \
     include/mpix/mpix_layout.h
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

src/transport/native.o: src/transport/pull_plan.h src/transport/layout.h \
                        src/transport/strided_plan.h src/transport/part_run.h \
                        src/transport/done_ring.h src/transport/pull_kernels.h \
                        src/transport/shm_ring.h src/transport/reduce.h \
                        src/transport/reduce_plan.h \
                        src/transport/strided_reduce_plan.h
src/enqueue.o src/partitioned.o: src/transport/layout.h src/transport/reduce.h

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(GPU_ARCH) $(OBJS) $(LDFLAGS) -o $@

clean:
	rm -f $(OBJS) $(LIB) $(PYEXT)

# Compile-validate the MPI-4.0 partitioned passthrough on this MPI-3.1
# toolchain (prototypes declared by internal.h under the forced gate; the
# objects are NOT linked into the library).  On a real MPI-4 library the
# gate turns on automatically — see internal.h.
# The scratch objects stay in-tree (build/ is ignored): a fixed name in a
# shared temp directory cannot be overwritten once another user has made it.
MPI4CHECK_DIR := build/mpi4check
mpi4check:
	mkdir -p $(MPI4CHECK_DIR)
	$(HIPCC) $(CXXFLAGS) -DMPIX_MPI_PARTITIONED -c src/partitioned.cpp -o $(MPI4CHECK_DIR)/part.o
	$(HIPCC) $(CXXFLAGS) -DMPIX_MPI_PARTITIONED -c src/transport/mpi.cpp -o $(MPI4CHECK_DIR)/mpi.o
	$(HIPCC) $(CXXFLAGS) -DMPIX_MPI_PARTITIONED -c src/enqueue.cpp -o $(MPI4CHECK_DIR)/enq.o
	@echo "mpi4check: MPI-4 partitioned passthrough compiles both ways"

# The check programs of the reducing receive: reduce.h and reduce_plan.h
# against independent references on the CPU (ASan + UBSan), and the reduce
# kernels launched directly on a GPU (tests/test_reduce_ref.py,
# tests/test_reduce_kernels_gpu.py).
reduce_check:
	$(MAKE) -C tools bin/reduce_check
	tools/bin/reduce_check

reduce_kernels_check:
	$(MAKE) -C tools bin/reduce_kernels_check

# The same for the strided reducing receive: strided_reduce_plan.h and
# layout_reduce_in on the CPU, the strided reduce kernels on a GPU
# (tests/test_strided_reduce_ref.py, tests/test_strided_reduce_kernels_gpu.py).
strided_reduce_check:
	$(MAKE) -C tools bin/strided_reduce_check
	tools/bin/strided_reduce_check

strided_reduce_kernels_check:
	$(MAKE) -C tools bin/strided_reduce_kernels_check

.PHONY: all clean python mpi4check reduce_check reduce_kernels_check \
        strided_reduce_check strided_reduce_kernels_check
