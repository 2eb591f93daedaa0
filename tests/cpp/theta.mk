# C++ host driver of the theta stepper surface (test harness): make -C tests/cpp -f theta.mk
OUT := ../_build/theta_driver
LIB := ../../i-emic_amd/lib
$(OUT): theta_driver.cpp ../../i-emic_amd/csrc/ocean.hpp ../../include/iemic.h $(LIB)/libiemic_amd.so
	@mkdir -p ../_build
	g++ -O2 -std=c++17 -o $@ theta_driver.cpp -L$(LIB) -liemic_amd -Wl,-rpath,'$$ORIGIN/../../i-emic_amd/lib'
